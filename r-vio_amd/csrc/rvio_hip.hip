// rvio_hip.hip — the C-ABI of include/rvio_hip.h: handle, HBM allocation, kernel sequencing.
// Single translation unit: the kernel files are included so that one hipcc call builds the whole library
// (the front end — frontend_kernels / klt3 / klt16 / clahe / detector — sits inside an FP-contraction-off region).
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <dlfcn.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rvio_hip.h"
#include "rvio_dev.h"
#include "ring_span.h"
#include "frontend_dev.h"
#include "filter_kernels.hip"
#include "filter_kernels2.hip"
#include "solve6.hip"
#include "solve7.hip"
#include "solve9.hip"   // round 5: the solve as blocked SPD factorisations on the matrix cores (one instance; every window up to 6n = 192)
#include "landmarks.hip"   // Updater::update's landmark cloud (rvio_hip_set_landmarks)
#include "landmark_cov.hip"   // the 3 x 3 covariance of every cloud point, behind landmark_kernel (rvio_hip_set_landmark_cov)
#include "odom.hip"        // the per-frame odometry record: pose, velocity, covariance (rvio_hip_set_odometry)
#include "imu_pose.hip"    // IMU-rate odometry: a pose per IMU sample (rvio_hip_predict, rvio_hip_set_imu_odometry)
#include "imu_cov.hip"     // ... and its covariance: pose_cov / vel_cov per IMU sample (rvio_hip_predict_cov, rvio_hip_set_imu_odometry_cov)
#include "aux_update.hip"  // the auxiliary measurement update: wheel odometry, zero velocity, speed over ground (rvio_hip_update_aux)
#include "standstill.hip"  // standstill detection in front of it: the zero-velocity update of the instances that do not move (rvio_hip_standstill)
#include "fix_rows.hip"    // absolute fixes in front of it: position, attitude, pose, gravity rows linearised at the current state (rvio_hip_update_fix)
#include "fix_past.hip"    // ... and delayed ones, linearised against the pose the clone window holds for the frame they were taken at (rvio_hip_update_fix_past)
#include "rel_rows.hip"    // relative poses between two frames of the window, linearised against the clones between them (rvio_hip_update_rel)
#include "window_pose.hip" // the fixed-lag smoothed trajectory: pose and covariance of every frame of the window (rvio_hip_get_window, rvio_hip_set_smoothed_odometry)
#include "window_edge.hip" // pose-graph export: the edge between two frames of the window and the joint covariance of its poses (rvio_hip_get_window_edges, rvio_hip_get_window_joint)
#pragma clang fp contract(off)
#include "frontend_kernels.hip"
#include "map_rows.hip"    // map landmarks: pixel observations of known world points at a past image, gated per point against P (rvio_hip_update_map)
#include "klt3.hip"
#include "klt16.hip"
#include "clahe.hip"
#include "detector.hip"
#include "gray.hip"        // Tracker.cc:182-196 for colour cameras (rvio_hip_set_image_format)
#include "raw.hip"         // ... and for 16-bit and Bayer cameras: cv_bridge's conversion to MONO8 (rvio_mono.cc:64)
#pragma clang fp contract(fast)

// A ring of records on the device, laid out as ring_span.h states (ring[(seq - 1) % cap][instance]); the operations on it follow the handle:
// ring_set_capacity, ring_read
template <typename T>
struct DevRing {
    const char *noun, *setter;   // for the error messages: "odometry", "rvio_hip_set_odometry"
    T* ring = nullptr;
    int cap = 0;           // records per instance the ring holds
    bool on = false;       // the launches that write it run
    long long seq = 0;     // records written since create / rvio_hip_initialize / the last change of capacity: the newest record's seq
    T* slot(long long s, int batch) const { return ring + ring_index(s, cap, batch); }   // the `batch` records of seq s
};
// The staging of one host-buffer entry point of the measurement updates: a pinned block the call packs, its device twin, and the event behind
// the H2D copy (the next call packs once that copy has left the pinned block).  Operations: stage_acquire, stage_send
struct HostStage { char* pin = nullptr; char* dev = nullptr; hipEvent_t ev = nullptr; };

struct rvio_hip {
    rvio_config cfg;
    DevCfg dc;
    int device = 0;
    hipStream_t stream = nullptr;     // filter stream (and the stream of every non-pipelined call)
    hipStream_t stream_t = nullptr;   // tracker stream of the pipelined whole-frame path
    hipEvent_t evT[4] = {nullptr, nullptr, nullptr, nullptr};   // book-keeping(k) done: a ring by frame number (the image chain of frame k waits for frame k-3's)
    hipEvent_t evH[4] = {nullptr, nullptr, nullptr, nullptr};   // hand-over of frame k written (bookkeep_a_kernel): what the filter of frame k waits for
    // Tracker -> Updater hand-over tables in rotation: book-keeping(k) rewrites table k % kHand once filter(k - kHand) has read it.  Two
    // tables (rounds 1-2) let the side chain run at most two frames ahead of the filter; four were built to absorb the frames in which the
    // side chain is late (one in ten: the gate in front of the filter then waits ~100 us).  Measured: they do not — the side chain's own
    // period equals the filter's (134 against 136 us in situ), so it never builds the lead; what is late in those frames is the IMAGE
    // chain (greedy_kernel: 29-200 us, data dependent), which the refill half of book-keeping waits for.  Kept: it costs 30 KB per instance.
    static const int kHand = 4;
    hipEvent_t evF[kHand] = {nullptr, nullptr, nullptr, nullptr}, evIn[2] = {nullptr, nullptr};
    long frame_no = 0;
    bool piped = false, in_frame = false;
    struct TrackOut { int* n_feat; unsigned char* types; int* len; float* meas; } tout[kHand];
    std::string err;
    // filter state (double-buffered)
    FilterMeta* meta = nullptr;
    double* x[2] = {nullptr, nullptr};
    double* P[2] = {nullptr, nullptr};
    int cur = 0;
    int img_count = 0;      // host mirror of nImageCountAfterInit (data-independent)
    int n_clones_host = 0;  // host mirror of nCloneStates (data-independent)
    int composed_count = 0; // img_count of the last frame whose augment / compose has run: the state's reference frame (img_count runs ahead of it between rvio_hip_frame_plan and rvio_hip_augment_compose)
    // update scratch
    double *partial = nullptr, *block = nullptr, *Ab = nullptr, *Tbuf = nullptr, *W = nullptr, *Mg = nullptr, *U = nullptr, *G = nullptr,
           *Pt1 = nullptr, *tm_global = nullptr, *gamma = nullptr, *pfinv = nullptr;
    int *nrows = nullptr, *acc = nullptr, *ndof = nullptr, *gram_cnt = nullptr;
    double* gpose = nullptr;   // batch handles (max_len <= 16): the pose chains geom4_kernel leaves for feat_build_kernel<4>, [Fu][(max_len-1) x 24]
    int* gvalid = nullptr;     // ... and the validity flag of each triangulation
    LaunchPlan plan;           // launch_plan.h: every LDS size and kernel variant that follows from (max_track_len, n_features, batch)
    // round 6 (literal.h): the rows of an update of <= LIT_FEATS features, exported by the per-feature kernel for the reference's literal sweep; the
    // state of the systolic array when it does not fit in the reduction's LDS (long windows, batch handles); nullptr: no literal path on this handle
    double *lit_rows = nullptr, *lit_state = nullptr;
    const double* last_Ab = nullptr;            // the [A|b] block of the last update (its meta row: frame_info)
    StageSync* stage_sync = nullptr;   // device-side completion counter of the filter chain (aug) and the value it reaches after the launches so far
    StageSync stage_tgt = {};
    double* S9scr = nullptr;     // solve9's slab of tiles in L2 (plan.solve9_nt != 0): 5 NT^2 x 256 doubles (+ the verdict of the Cholesky role)
    bool chol_ready = false;     // the slab holds L, G of the clone block the next solve will see (written by the role workgroup of the per-feature / propagate launch).
                                 // chol_ready / chol_async: touched by the chol_* functions only, see the rule above them
    float* eig_map = nullptr;    // W x H min-eigenvalue map of rvio_hip_get_corners(eig): allocated on first use
    // staging
    rvio_imu* d_imu = nullptr;
    double* gathered = nullptr;   // rvio_hip_frame_sharded_dev: world x [S2 | S1] as the all-gather delivers them (allocated on first use)
    int gathered_world = 0;
    int imu_cap = RVIO_MAX_IMU;   // samples the host-side staging (d_imu, hb_imu, pinned ring) holds; grows on demand (ensure_imu_capacity)
    float* d_cand = nullptr;
    uint8_t* d_img = nullptr;
    static const int kIC = 3;                     // image chains in flight in run-ahead mode (streams, detector scratch sets, CLAHE LUT sets)
    DetDev dets[kIC] = {};                        // device detector (T7), allocated on first use: kIC sets of scratch — in run-ahead mode the
                                                  // detectors of consecutive frames run on two streams, by frame parity
    bool det_ready = false;
    hipStream_t stream_l = nullptr;               // long windows (6n > 96): = stream_c (one image chain in flight); the Cholesky factor of the clone block runs here, beside propagate / the per-feature stage of the frame it serves
    hipEvent_t evA = nullptr, evL = nullptr;      // augment/compose done (filter stream) -> stream_l;  factor in the slab (stream_l) -> the solve
    bool chol_async = false;                      // a factor of the CURRENT clone block is in flight on (or has left) stream_l
    hipStream_t stream_d = nullptr;               // side stream of the front end: forks from / joins the tracker stream (see build_pyramid_dev)
    hipStream_t stream_c = nullptr;               // CLAHE stream of the run-ahead mode (frame k+1 is equalised while frame k is still being detected)
    hipEvent_t evC[kIC] = {nullptr, nullptr, nullptr};   // equalised image + pyramid of the frame ready, by image chain
    hipEvent_t evD0 = nullptr, evD1 = nullptr;
    uint8_t* hb_img[2] = {nullptr, nullptr};      // staging of rvio_hip_frame (host buffers), by frame parity
    rvio_imu* hb_imu[kHand + 1] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // (run-ahead mode rotates kHand + 1 slots: see rvio_hip_frame)
    // how "the filter of the frame with parity b has finished" is known: 0 = evF[b] was recorded behind it, 1 = the device-side counter
    // stage_sync->aug reaches fin_target[b] (single instance, run-ahead mode: no marker packet on the filter stream)
    int fin_mode[kHand] = {0, 0, 0, 0};
    unsigned long long fin_target[kHand] = {0, 0, 0, 0};
    bool last_ra = false;             // the previous rvio_hip_frame call ran in run-ahead mode
    float* hb_cand[2] = {nullptr, nullptr};
    // pinned host ring of rvio_hip_frame: the caller's (pageable) buffers are packed into it on the host, the H2D copies then run
    // asynchronously from pinned memory.  Slot s may be refilled once evPin[s] (recorded behind its copies) has completed.
    static const int kPin = 3;
    uint8_t* pin[kPin] = {nullptr, nullptr, nullptr};
    hipEvent_t evPin[kPin] = {nullptr, nullptr, nullptr}, evPin2[kPin] = {nullptr, nullptr, nullptr};
    size_t pin_img = 0, pin_imu = 0, pin_bytes = 0;
    uint8_t *d_eq = nullptr, *d_lut2[kIC] = {nullptr, nullptr, nullptr};   // CLAHE output image and tile LUTs (enable_equalizer), the LUTs by image chain
    // Buffers the front end of frame k+1 would otherwise overwrite while book-keeping of frame k still reads them (run-ahead of the
    // image chain on the pipelined path, see track_dev_impl): equalised image, detector corner list and its count, by frame parity
    uint8_t* d_eq2[4] = {nullptr, nullptr, nullptr, nullptr};   // four, in rotation: the equalised image IS level 0 of its pyramid, which the KLT of the NEXT frame still reads
    int eq_slot = 0;
    float* det_xy2[3] = {nullptr, nullptr, nullptr};   // corner lists: by parity, in run-ahead mode three in rotation (FrontForms::dslot)
    int* det_nout = nullptr;
    // What the getters and rvio_hip_debug_time_kernel need to know about the LAST front-end call, written when that call has enqueued its launches.  (The
    // mode of a call in progress is no handle state: it is the FrontForms value the call computes once and passes down.)
    struct Last {
        int dslot = 0;                            // its corner list / count (rvio_hip_get_corners)
        int det_set = 0;                          // the detector scratch set it used
        const uint8_t* gray_src = nullptr; int gray_stride = 0; size_t gray_bs = 0;   // the last colour image handed over (rvio_hip_debug_time_kernel(11))
    } last;
    bool private_queues = false;                  // this handle's streams own hardware queues (make_stream)
    bool queues_shared = false;                   // ... unless one of them had to come from the shared pool after all
    bool extra_queues = false;                    // a collective's queues run beside this handle's (rvio_hip_frame_sharded_dev with a communicator)
    int cl_tx = 0, cl_ty = 0, cl_tw = 0, cl_th = 0, cl_clip = 0;
    float cl_scale = 0.f;
    float* d_in_xy = nullptr;
    unsigned char* d_in_st = nullptr;
    // tracker
    TrackerDev t;
    PyrDev pyr[4];   // four in rotation: pyramid(k) (image stream, run-ahead) may be built while KLT(k-2), KLT(k-1) still match the others
    int pyr_cur = 0;
    // Everything allocated outside the slab — the slab itself, the on-demand buffers of the features, pinned staging, their events — belongs to
    // this registry (own_dev / own_pinned / own_event, own_replace, own_release); rvio_hip_destroy walks it, no member is freed by name
    struct Owned { void* p; int kind; };   // kind: OWN_DEV | OWN_PINNED | OWN_EVENT
    std::vector<Owned> owned;
    // filter slab: the filter state, the update scratch and the Tracker -> Updater hand-over of ONE instance are carved from one
    // slab; a batch handle (rvio_hip_create_batch) owns `batch` slabs back to back and launches every filter kernel with
    // gridDim.z = batch (rvio_dev.h zoff)
    char* slab = nullptr;
    size_t slab_off = 0, slab_bytes = 0;
    bool slab_mode = false;
    int batch = 1;
    const rvio_imu* fuse_imu = nullptr;   // whole-frame path: propagate of this frame rides in the per-feature launch (feat_prop_kernel)
    const rvio_imu* time_imu = nullptr; int time_m = 0;   // the IMU batch of the last fused frame (rvio_hip_debug_time_kernel(8) only: the caller's buffer)
    int fuse_m = -1;                      // >= 0 while such a propagate is pending
    bool wide_px = false;            // throughput forms of the image kernels (several pixels per thread): batch handles of >= 8 instances.  An INPUT of front_forms(), read nowhere else
    bool front_end = true;           // a batch handle may carry the filter only
    bool det_in_slab = false;        // batch handle with front end: the detector's buffers are slab members too
    size_t img_bs = 0, imu_bs = 0;   // instance strides (bytes) of the image / IMU batch of the call in progress
    BatchIn bin = {0, 0, 0, 0, 0};   // strides of the hand-over read by feat_build (slab_bytes for the handle's own buffers)
    int* rng = nullptr;
    int* first_mirror = nullptr;     // pinned, device-mapped: mbIsTheFirstImage of every instance as book-keeping leaves it
    bool first_cleared = false;      // (cached) every instance has seen its first image: nms(k+1) need not wait for book-keeping(k)
    int* cand_scratch = nullptr;
    rvio_frame_info* d_info = nullptr;
    double* d_pose = nullptr;
    // landmark cloud of the last update (landmark_kernel): allocated on the first rvio_hip_set_landmarks(1), outside the filter slab (a handle
    // that never enables it keeps its memory layout); one cloud per instance, lm.bs bytes apart
    bool lm_on = false;
    int lm_frame = -1;       // nImageCountAfterInit when the update behind the cloud was enqueued, -1: none since create / initialize
    LmOut lm = {nullptr, nullptr, nullptr, nullptr, 0};
    // landmark covariance (landmark_cov_kernel behind landmark_kernel): Fu records per instance, allocated on the first rvio_hip_set_landmark_cov(1)
    bool lmc_on = false;
    int lmc_frame = -1;      // lm_frame of the last cloud the records describe, -1: none since create / initialize
    rvio_landmark_cov* lmc = nullptr;
    // odometry ring (odom_kernel behind every augment/compose stage): allocated by rvio_hip_set_odometry, outside the slab (a handle that never
    // enables it keeps its memory layout and its launches)
    DevRing<rvio_odom> odom{"odometry", "rvio_hip_set_odometry"};
    // smoothed-odometry ring (window_pose_kernel behind odom_kernel's place in every augment/compose stage, the record of age smo_lag): allocated by
    // rvio_hip_set_smoothed_odometry, outside the slab.  win_buf: the staging of rvio_hip_get_window (nmax + 1 records), allocated by its first call
    DevRing<rvio_window_pose> smo{"smoothed-odometry", "rvio_hip_set_smoothed_odometry"};
    int smo_lag = 0;
    rvio_window_pose* win_buf = nullptr;
    // edge-odometry ring (window_edge_kernel behind the smoothed record's place, the pair (edg_new, edg_old)): allocated by
    // rvio_hip_set_edge_odometry, outside the slab.  wedge_buf: the staging of rvio_hip_get_window_edges (LP_WEDGE_MAX_PAIRS records, then the two
    // age lists); wjoint_buf: that of rvio_hip_get_window_joint ((6 (nmax + 1))^2 doubles, then nmax + 1 pose records); each allocated by the first call
    DevRing<rvio_window_edge> edg{"edge-odometry", "rvio_hip_set_edge_odometry"};
    int edg_new = 0, edg_old = 1;
    char* wedge_buf = nullptr;
    char* wjoint_buf = nullptr;
    // IMU-rate ring (imu_pose_kernel in front of whatever propagates in place): allocated by rvio_hip_set_imu_odometry, outside the slab;
    // imuo.seq counts the samples recorded (the m of every propagate while the ring is on)
    DevRing<rvio_imu_pose> imuo{"IMU-rate odometry", "rvio_hip_set_imu_odometry"};
    // its covariance ring (imu_cov_kernel next to imu_pose_kernel): allocated by rvio_hip_set_imu_odometry_cov, outside the slab, with imuo's capacity,
    // seq and slot rule.  imuc.seq: the newest record written; imuc_first: the first one since covariance was last switched on
    DevRing<rvio_imu_cov> imuc{"IMU-rate covariance", "rvio_hip_set_imu_odometry_cov"};
    long long imuc_first = 1;
    size_t time_imu_bs = 0;    // instance stride of time_imu (rvio_hip_debug_time_kernel(13), (14))
    // staging of rvio_hip_predict / rvio_hip_predict_cov (host in / host out), outside the slab, owned by predict_staging: samples in, records out
    struct PredStage { rvio_imu* imu = nullptr; rvio_imu_pose* out = nullptr; rvio_imu_cov* cov = nullptr; int cap = 0; } pred;
    bool has_state = false;    // rvio_hip_set_state* / rvio_hip_initialize* has run (rvio_hip_predict* refuses to extrapolate from nothing)
    // auxiliary measurement update (aux_update.hip), allocated by the first rvio_hip_update_aux* call, outside the slab: (gamma, applied) of the
    // last call per instance; the host form's staging [H | v | sigma | active flags]
    struct { double* diag = nullptr; HostStage stage; } aux;
    // standstill detection (standstill.hip): the configuration of rvio_hip_set_standstill; one block allocated by the first rvio_hip_standstill*
    // call, outside the slab — records, (gamma, applied) pairs of ITS aux launches, v (6 per instance), the shared H (6 x dmax) and sigma, the
    // flags — the staging of the host-buffer form, and the two events that order the detector against the filter stream.
    // book_stream: the stream that ran the last book-keeping (post_klt_dev), where the detector is launched; ss_last: the stream the last detector
    // ran on while no book-keeping has been enqueued behind it (nullptr otherwise): a book-keeping on ANOTHER stream waits for evSSb first
    bool ss_on = false;
    rvio_standstill_config ss_cfg = {};
    rvio_standstill* ss_rec = nullptr;
    double *ss_diag = nullptr, *ss_v = nullptr, *ss_H = nullptr, *ss_sigma = nullptr;
    int* ss_active = nullptr;
    rvio_imu* ss_imu = nullptr;
    int ss_imu_cap = 0;
    hipEvent_t evSSa = nullptr, evSSb = nullptr;
    hipStream_t book_stream = nullptr, ss_last = nullptr;
    // absolute fixes (fix_rows.hip): one block allocated by the first rvio_hip_update_fix* call, outside the slab — the rows H (6 x dmax per
    // instance), r and sigma (6 per instance), the records, the (gamma, applied) pairs of ITS aux launches — and the host form's staging (one
    // rvio_fix, one flag per instance).  kind / m / d: the last call's, for the getters
    struct {
        double *H = nullptr, *r = nullptr, *sigma = nullptr, *pair = nullptr;
        rvio_fix_diag* rec = nullptr;
        HostStage stage;
        int kind = 0, m = 0, d = 0;
    } fx;
    // past-frame fixes (fix_past.hip) reuse that block and add, with the first rvio_hip_update_fix_past* call, the kernel's flags (one int32 per
    // instance) and the host form's staging (one rvio_fix; frac, age and flag per instance)
    struct { int32_t* flag = nullptr; HostStage stage; } fp;
    // relative-pose measurements (rel_rows.hip) reuse the fix block and the kernel's flags of the past-frame fixes, and add, with the first
    // rvio_hip_update_rel call, the host form's staging (one rvio_fix; age_new, age_old and flag per instance)
    struct { HostStage stage; } rl;
    // map landmarks (map_rows.hip): a block of their own, allocated with the first rvio_hip_update_map* call — rows (LP_MAP_ROWS x dmax per
    // instance), r, sigma, the (gamma, applied) pairs, the records, the per-slot records, the kernel's flags — and the host form's staging
    // (RVIO_MAP_MAX_POINTS records; age and flag per instance).  m, d: the rows of the last call, for the getters
    struct { double* H = nullptr; double* r = nullptr; double* sigma = nullptr; double* pair = nullptr; rvio_map_diag* rec = nullptr; rvio_map_point* pts = nullptr;
             int32_t* flag = nullptr; int m = 0, d = 0; HostStage stage; } mp;
    // iterated measurement updates (rvio_hip_set_meas_iterations): the setting, and one block allocated by the first iterated call, outside the
    // slab — per instance the snapshot (launch_plan.h meas_iter_x0_stride doubles), dx (dmax doubles), the record, the running flag.
    // last_pair: the (gamma, applied) pairs of the last fix / past-fix / rel / map call (nullptr: none yet); last_iterated: it ran the chain
    struct { int max_iters = 1; double tol = 0.0; double* x0 = nullptr; double* dx = nullptr; rvio_meas_iter* rec = nullptr; int32_t* run = nullptr;
             const double* last_pair = nullptr; bool last_iterated = false; } mi;
    // colour input (rvio_hip_set_image_format): the gray images every stage behind gray_kernel reads instead of the caller's.  Allocated with the
    // first colour format, outside the slab (a mono handle keeps its memory layout), instance stride W * H; four in rotation like d_eq2[] (see
    // build_pyramid_dev for who reads a slot last)
    int pix_fmt = RVIO_PIX_MONO8, pix_ch = 1;   // pix_ch: BYTES per pixel as staged (samples per pixel x bytes per sample)
    uint8_t* d_gray[4] = {nullptr, nullptr, nullptr, nullptr};
    int gray_slot = 0;
    // per-instance calibration (rvio_hip_set_calibration*): `cals` is what the getter returns, one entry per instance, the config's until a setter
    // changes it; `cal` is the device table the calibrated kernels index by instance, allocated by the FIRST setter, outside the slab — a
    // handle that never calls one passes nullptr and its kernels read DevCfg::cam from their arguments, as before the table existed
    std::vector<rvio_calibration> cals;
    CamCal* cal = nullptr;
    size_t img_cap = 0;              // bytes of one staged image the host-side staging (d_img, hb_img[]) holds: W * H, grows with the channel count
};

// ---------------------------------------------------------------- environment surface of the library: three variables of its own, plus the profiler's.
//   RVIO_PARANOID     every cross-queue hand-off in its most conservative form (A/B against the default, and the thing to set when a
//                     runtime / firmware is suspected).  "1" = all of it; a larger value is a bit mask for bisection:
//                       2  events with the default flags (system-scope release at every record) instead of hipEventDisableSystemFence
//                       4  no device-side polls: every hand-off is a stream-level event (no StageSync counters, no gate / signal kernels)
//                       8  plain hipStreamCreateWithFlags(hipStreamNonBlocking) streams instead of CU-mask streams with private queues
//                      16  rvio_hip_frame waits on the host for its H2D staging copies before it enqueues the frame
//                      32  every whole-frame call drains all streams of the handle before it returns
//   RVIO_NO_RUNAHEAD  the pipelined path without the run-ahead image chains (book-keeping back on the tracker stream)
//   RVIO_NO_LITERAL   no literal sweep: the structural rank rule alone, as up to round 5 (read when a handle is created)
//   ROCPROF_COUNTER_COLLECTION  (exported by rocprofv3 --pmc) a counter-collecting profiler serialises kernels across queues: no device-side polls
// Kernel forms and stream layouts follow from what the code observes (window length, batch size, the LDS budget of launch_plan.h), never from
// the environment; the instrumented build (-DRVIO_DBG_CLOCKS, tools/chain_clocks.py) launches what the shipping build launches and adds its
// stamps (and RVIO_DBG_HOST, which prints host-side enqueue times and selects nothing).
enum { PAR_SYSFENCE = 2, PAR_NO_DEVPOLL = 4, PAR_PLAIN_STREAMS = 8, PAR_SYNC_COPIES = 16, PAR_DRAIN = 32, PAR_ALL = 62 };
static int paranoid_bits() {
    static const int v = [] {
        const char* e = getenv("RVIO_PARANOID");
        if (!e || !*e || !std::strcmp(e, "0")) return 0;
        const int b = atoi(e);
        return b > 1 ? (b & PAR_ALL) : (int)PAR_ALL;
    }();
    return v;
}
static bool no_runahead() {
    static const bool v = getenv("RVIO_NO_RUNAHEAD") != nullptr;
    return v;
}
// The handle's events only order kernels of ONE device across its streams; the host only ever WAITS for them (hipEventSynchronize on the
// pinned ring's events, hipStreamSynchronize elsewhere): no timing, and no system-scope fence when they are recorded — that fence writes the
// dirty L2 lines of the recording queue back before the NEXT kernel of that queue may start (measured: a 35 us hole in the tracker stream per frame)
static unsigned ev_flags() { return (paranoid_bits() & PAR_SYSFENCE) ? hipEventDisableTiming : (hipEventDisableTiming | hipEventDisableSystemFence); }
#define kEvFlags ev_flags()
#define HIPCHK(h, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
            return RVIO_ERR_NO_DEVICE;                                                           \
        }                                                                                        \
    } while (0)

// a step that returns an RVIO_* code of its own (and has set h->err): pass a failure on
#define RCCHK(call)                                   \
    do {                                              \
        const int rc_ = (call);                       \
        if (rc_ != RVIO_OK) return rc_;               \
    } while (0)

// ---------------------------------------------------------------- the registry of what the handle owns outside the slab (rvio_hip::owned).
// Each allocation writes *p only when it has succeeded, so a set-up of several parts allocates into locals and commits its members last.
enum { OWN_DEV, OWN_PINNED, OWN_EVENT };
// a device block; zero: cleared on the filter stream (the caller waits for that stream before another stream uses the block)
template <typename T>
static int own_dev(rvio_hip* h, T** p, size_t bytes, bool zero = false) {
    void* q = nullptr;
    HIPCHK(h, hipMalloc(&q, bytes));
    h->owned.push_back({q, OWN_DEV});
    if (zero) HIPCHK(h, hipMemsetAsync(q, 0, bytes, h->stream));
    *p = (T*)q;
    return RVIO_OK;
}
template <typename T>
static int own_pinned(rvio_hip* h, T** p, size_t bytes, unsigned flags = hipHostMallocDefault) {
    void* q = nullptr;
    HIPCHK(h, hipHostMalloc(&q, bytes, flags));
    h->owned.push_back({q, OWN_PINNED});
    *p = (T*)q;
    return RVIO_OK;
}
static int own_event(rvio_hip* h, hipEvent_t* e, unsigned flags) {
    hipEvent_t q = nullptr;
    HIPCHK(h, hipEventCreateWithFlags(&q, flags));
    h->owned.push_back({(void*)q, OWN_EVENT});
    *e = q;
    return RVIO_OK;
}
static void own_free(const rvio_hip::Owned& o) {
    if (o.kind == OWN_DEV) (void)hipFree(o.p);
    else if (o.kind == OWN_PINNED) (void)hipHostFree(o.p);
    else (void)hipEventDestroy((hipEvent_t)o.p);
}
// frees a block / destroys an event NOW: the caller knows that nothing in flight uses it.  nullptr: nothing to do
static void own_release(rvio_hip* h, void* p) {
    for (auto it = h->owned.begin(); it != h->owned.end(); ++it)
        if (it->p == p) { own_free(*it); h->owned.erase(it); return; }
}
// a block of another size in the place of *p: the new one first (a failure leaves *p as it was), then the old one is freed
template <typename T>
static int own_replace(rvio_hip* h, T** p, size_t bytes) {
    T* const old = *p;
    RCCHK(own_dev(h, p, bytes));
    own_release(h, old);
    return RVIO_OK;
}
// Registry entries that live as long as one call (the temporaries of the debug hooks): released when the scope ends, on every path out of it
// — behind a wait for the filter stream, on which the hooks use them
struct OwnedScope {
    rvio_hip* h;
    std::vector<void*> held;
    explicit OwnedScope(rvio_hip* h_) : h(h_) {}
    template <typename T> int dev(T** p, size_t bytes) { const int rc = own_dev(h, p, bytes); if (rc == RVIO_OK) held.push_back(*p); return rc; }
    int event(hipEvent_t* e, unsigned flags) { const int rc = own_event(h, e, flags); if (rc == RVIO_OK) held.push_back(*e); return rc; }
    ~OwnedScope() { (void)hipStreamSynchronize(h->stream); for (void* p : held) own_release(h, p); }
};

template <typename T>
static int dalloc(rvio_hip* h, T** p, size_t n) {
    size_t bytes = n * sizeof(T);
    if (bytes == 0) bytes = 16;
    if (h->slab_mode) {   // bump allocation inside the filter slab (first pass, slab == nullptr: sizes only)
        *p = h->slab ? (T*)(h->slab + h->slab_off) : nullptr;
        h->slab_off += (bytes + 255) & ~(size_t)255;
        return RVIO_OK;
    }
    return own_dev(h, p, bytes, true);
}
// entry points that address ONE instance's front end (a batch handle is driven by rvio_hip_frame_batch_dev / _frame_tracks_dev)
#define FRONT_END_ONLY(h)                                                                                              \
    do {                                                                                                               \
        if ((h)->batch > 1) { (h)->err = "single-instance entry point called on a batch handle"; return RVIO_ERR_UNSUPPORTED; } \
    } while (0)
#define SYNC_FRONT(h)                                                                     \
    do {                                                                                  \
        if ((h)->stream_c) HIPCHK(h, hipStreamSynchronize((h)->stream_c));                \
        if ((h)->stream_d) HIPCHK(h, hipStreamSynchronize((h)->stream_d));                \
        HIPCHK(h, hipStreamSynchronize((h)->stream_t));                                   \
    } while (0)
#define DALLOC(h, p, n) RCCHK(dalloc((h), &(p), (n)))

extern "C" {

int rvio_hip_abi_version(void) { return RVIO_HIP_ABI_VERSION; }

// config/rvio_euroc.yaml:8-111
void rvio_config_euroc(rvio_config* c) {
    std::memset(c, 0, sizeof *c);
    c->imu_rate = 200;
    c->sigma_g = 1.6968e-04; c->sigma_wg = 1.9393e-05; c->sigma_a = 2.0e-3; c->sigma_wa = 3.0e-3;
    c->gravity = 9.8082; c->small_angle = 0.001745329;
    c->width = 752; c->height = 480;
    c->fx = 458.654f; c->fy = 457.296f; c->cx = 367.215f; c->cy = 248.375f;
    c->k1 = -0.28340811f; c->k2 = 0.07395907f; c->p1 = 0.00019359f; c->p2 = 1.76187114e-05f; c->k3 = 0.f;
    c->sigma_px = 0.002180293f; c->sigma_py = 0.002186767f;
    const double T[16] = {0.0148655429818, -0.999880929698, 0.00414029679422, -0.0216401454975,
                          0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768,
                          -0.0257744366974, 0.00375618835797, 0.999660727178, 0.00981073058949,
                          0.0, 0.0, 0.0, 1.0};
    std::memcpy(c->T_bc, T, sizeof T);
    c->fisheye = 0;
    c->n_features = 200; c->max_track_len = 15; c->min_track_len = 3;
    c->min_dist = 15; c->qual_lvl = 0.01f; c->block_x = 150; c->block_y = 120;
    c->enable_equalizer = 1; c->use_sampson = 1; c->inlier_thr = 1e-5;
    c->ini_thr_angle = 0.005; c->ini_thr_displ = 0.01; c->ini_enable_alignment = 1;
}

void rvio_calibration_from_config(const rvio_config* c, rvio_calibration* k) {
    if (!c || !k) return;
    std::memset(k, 0, sizeof *k);
    k->fx = c->fx; k->fy = c->fy; k->cx = c->cx; k->cy = c->cy;
    k->k1 = c->k1; k->k2 = c->k2; k->p1 = c->p1; k->p2 = c->p2; k->k3 = c->k3;
    k->fisheye = c->fisheye;
    std::memcpy(k->T_bc, c->T_bc, sizeof k->T_bc);
}
// the device form of one calibration: the ONE place it is computed (the config's at create, a setter's later: the same bits either way)
static void fill_camcal(const rvio_calibration* c, CamCal* d) {
    std::memset(d, 0, sizeof *d);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) { d->Ric[3 * i + j] = c->T_bc[4 * i + j]; d->Rci[3 * j + i] = c->T_bc[4 * i + j]; }
        d->tic[i] = c->T_bc[4 * i + 3];
    }
    for (int i = 0; i < 3; ++i) d->tci[i] = -(d->Rci[3 * i] * d->tic[0] + d->Rci[3 * i + 1] * d->tic[1] + d->Rci[3 * i + 2] * d->tic[2]);
    d->fx = c->fx; d->fy = c->fy; d->cx = c->cx; d->cy = c->cy;
    d->k1 = c->k1; d->k2 = c->k2; d->p1 = c->p1; d->p2 = c->p2; d->k3 = c->k3;
    d->fisheye = c->fisheye ? 1 : 0;
}

static void fill_devcfg(const rvio_config* c, DevCfg* d) {
    std::memset(d, 0, sizeof *d);
    d->gravity = c->gravity; d->small_angle = c->small_angle;
    d->sg2 = c->sigma_g * c->sigma_g; d->swg2 = c->sigma_wg * c->sigma_wg;
    d->sa2 = c->sigma_a * c->sigma_a; d->swa2 = c->sigma_wa * c->sigma_wa;
    d->sigma_im = (double)std::max(c->sigma_px, c->sigma_py);   // float max, widened (Updater.cc:42-44)
    d->inlier_thr = c->inlier_thr;
    { rvio_calibration k; rvio_calibration_from_config(c, &k); fill_camcal(&k, &d->cam); }
    d->W = c->width; d->H = c->height;
    d->F = c->n_features; d->Fu = (int)std::ceil(.5 * c->n_features);
    d->max_len = c->max_track_len; d->min_len = c->min_track_len;
    d->nmax = c->max_track_len - 1; d->dmax = 24 + 6 * d->nmax; d->xdmax = 26 + 7 * d->nmax;
    d->rho_max = 2 * c->max_track_len - 2;
    d->ldh = 6 * d->nmax + 1;
    // FeatureDetector ctor, FeatureDetector.cc:29-52
    d->min_dist = c->min_dist;
    d->block_x = c->block_x; d->block_y = c->block_y;
    // (mnGridCols/Rows, mnOffsetX/Y and mnMaxFeatsPerBlock are `int` members upstream: the assignments truncate, FeatureDetector.h:66-77)
    d->grid_cols = (int)std::floor(c->width / c->block_x);
    d->grid_rows = (int)std::floor(c->height / c->block_y);
    d->off_x = (float)(int)(.5 * (c->width - d->grid_cols * c->block_x));
    d->off_y = (float)(int)(.5 * (c->height - d->grid_rows * c->block_y));
    d->max_per_block = (d->grid_cols * d->grid_rows > 0) ? (float)(int)((float)c->n_features / (d->grid_cols * d->grid_rows)) : 0.f;
    d->use_sampson = c->use_sampson;
    // buildOpticalFlowPyramid: stop when a level is not larger than the window
    int w = c->width, hgt = c->height, lv = 1;
    for (int l = 1; l <= 3; ++l) { w = (w + 1) / 2; hgt = (hgt + 1) / 2; if (w <= 15 || hgt <= 15) break; lv++; }
    d->levels = lv;
}

// The per-instance filter buffers (state, update scratch, Tracker -> Updater hand-over, IMU staging): called twice — sizes, then pointers
static int alloc_filter_slab(rvio_hip* h) {
    const DevCfg& d = h->dc;
    const size_t dm = d.dmax, PP = dm * dm, ldh = d.ldh;
    TrackerDev& t = h->t;
    DALLOC(h, h->meta, 1);
    for (int b = 0; b < 2; ++b) { DALLOC(h, h->x[b], (size_t)d.xdmax + 8); DALLOC(h, h->P[b], PP); }
    DALLOC(h, h->partial, (size_t)d.Fu * ldh * ldh);   // per-feature shares G_f = Hn^T [Hn | r] of the information block
    DALLOC(h, h->block, 2 * ldh * ldh);   // [S2 | S1]: the type-'2' and type-'1' sums of the information block (gram_reduce_kernel)
    DALLOC(h, h->Ab, 2 * ldh * ldh);
    DALLOC(h, h->gram_cnt, 8);
    DALLOC(h, h->stage_sync, 1);
    DALLOC(h, h->Tbuf, ldh * ldh); DALLOC(h, h->W, ldh * ldh);
    DALLOC(h, h->U, dm * ldh); DALLOC(h, h->G, dm * ldh);
    DALLOC(h, h->Pt1, PP);
    DALLOC(h, h->gamma, d.Fu); DALLOC(h, h->pfinv, (size_t)3 * d.Fu);
    DALLOC(h, h->nrows, d.Fu); DALLOC(h, h->acc, d.Fu); DALLOC(h, h->ndof, d.Fu);
    DALLOC(h, h->d_imu, RVIO_MAX_IMU);
    DALLOC(h, h->d_info, 1); DALLOC(h, h->d_pose, 8);
    DALLOC(h, t.n_feat, 1); DALLOC(h, t.types, d.Fu); DALLOC(h, t.len, d.Fu); DALLOC(h, t.meas, (size_t)2 * d.Fu * d.max_len);
    if (h->plan.tm_global) DALLOC(h, h->tm_global, (size_t)d.Fu * d.rho_max * ldh);
    static const bool no_lit = getenv("RVIO_NO_LITERAL") != nullptr;   // A/B: the structural rank rule alone, as up to round 5
    if (!no_lit && h->plan.lit_ok) {
        DALLOC(h, h->lit_rows, lit_rows_doubles(d.ldh, d.rho_max));
        if (h->plan.lit_state_global) DALLOC(h, h->lit_state, lit_state_doubles(d.ldh - 1));
    }
    if (h->batch > 1 && d.max_len <= GEOM4_ML) { DALLOC(h, h->gpose, (size_t)d.Fu * (d.max_len - 1) * 24); DALLOC(h, h->gvalid, d.Fu); }
    return RVIO_OK;
}

static int detector_alloc(rvio_hip* h);
static int detector_check(rvio_hip* h);
// The per-instance front-end buffers (staging, CLAHE, tracker tables, two pyramids; the detector's for a batch handle)
static int alloc_frontend_slab(rvio_hip* h) {
    const DevCfg& d = h->dc;
    TrackerDev& t = h->t;
    DALLOC(h, h->d_cand, (size_t)2 * d.F);
    DALLOC(h, h->d_img, (size_t)d.W * d.H);
    if (h->cfg.enable_equalizer) {
        DALLOC(h, h->d_eq2[0], (size_t)d.W * d.H); DALLOC(h, h->d_eq2[1], (size_t)d.W * d.H); DALLOC(h, h->d_eq2[2], (size_t)d.W * d.H);
        DALLOC(h, h->d_eq2[3], (size_t)d.W * d.H);
        h->d_eq = h->d_eq2[0];
        for (int k = 0; k < std::max(2, h->plan.n_ic); ++k) DALLOC(h, h->d_lut2[k], (size_t)h->cl_tx * h->cl_ty * 256);
    }
    DALLOC(h, h->d_in_xy, (size_t)2 * d.F); DALLOC(h, h->d_in_st, d.F);
    DALLOC(h, h->rng, 40); DALLOC(h, h->cand_scratch, (size_t)2 * d.F + 8);
    DALLOC(h, t.first, 1); DALLOC(h, t.n_pts, 1);
    DALLOC(h, t.feats, (size_t)2 * d.F); DALLOC(h, t.un1, (size_t)2 * d.F); DALLOC(h, t.slot, d.F);
    DALLOC(h, t.hist, (size_t)2 * d.F * d.max_len); DALLOC(h, t.hist_len, d.F);
    DALLOC(h, t.tracked, (size_t)2 * d.F); DALLOC(h, t.un2, (size_t)2 * d.F); DALLOC(h, t.status, d.F);
    DALLOC(h, t.tmp_feats, (size_t)2 * d.F); DALLOC(h, t.tmp_un, (size_t)2 * d.F); DALLOC(h, t.tmp_slot, d.F);
    DALLOC(h, t.cand_acc, d.F); DALLOC(h, t.mid, 4);
    DALLOC(h, t.cell_pts, (size_t)d.grid_cols * d.grid_rows * 2 * d.F * 2);
    for (int k = 1; k < rvio_hip::kHand; ++k) {
        DALLOC(h, h->tout[k].n_feat, 1); DALLOC(h, h->tout[k].types, d.Fu); DALLOC(h, h->tout[k].len, d.Fu);
        DALLOC(h, h->tout[k].meas, (size_t)2 * d.Fu * d.max_len);
    }
    for (int b = 0; b < 4; ++b) {
        int w = d.W, hg = d.H;
        for (int l = 0; l < 4; ++l) {
            uint8_t* im = nullptr; short* dx = nullptr;   // (no derivative images: the KLT kernel forms them from its staged patch)
            if (l < d.levels) DALLOC(h, im, (size_t)w * hg);
            h->pyr[b].img[l] = im; h->pyr[b].dxy[l] = dx; h->pyr[b].w[l] = w; h->pyr[b].h[l] = hg;
            w = (w + 1) / 2; hg = (hg + 1) / 2;
        }
    }
    if (h->det_in_slab) return detector_alloc(h);
    return RVIO_OK;
}

// The four streams of a handle each need a hardware queue of their own: the run-ahead pipeline is four concurrent chains, and two of them
// on one queue serialise (measured: 4.5 k instead of 6.6 k frames/s).  hipStreamCreate deals streams onto a pool of GPU_MAX_HW_QUEUES (4)
// shared queues by reference count, so whether a handle gets four distinct ones depends on every stream the process created before it
// (torch's, another library's).  A stream created with a CU mask owns a private queue; the mask here enables every CU.
// ... for ONE handle: beyond four busy queues the command processor time-slices (eight handles with four private queues each ran at a quarter
// of the rate of eight handles on the shared pool), so only the first live handle of a process takes private queues; the others share the pool
// as before (many streams per GPU are what batch handles are for).
static std::atomic<int> g_private_queue_handles{0};
static hipError_t make_stream(rvio_hip* h, hipStream_t* s) {
    if ((paranoid_bits() & PAR_PLAIN_STREAMS) || !h->private_queues) { h->queues_shared = true; return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, h->device);
    if (e != hipSuccess) return e;
    const int words = (prop.multiProcessorCount + 31) / 32;
    std::vector<uint32_t> mask((size_t)std::max(words, 1), 0xffffffffu);
    if (prop.multiProcessorCount % 32) mask.back() = (1u << (prop.multiProcessorCount % 32)) - 1u;
    e = hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data());
    if (e != hipSuccess) { (void)hipGetLastError(); h->queues_shared = true; return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
    return e;
}

static bool profiler_serialises() {
    const char* e = getenv("ROCPROF_COUNTER_COLLECTION");
    return e && *e && std::strcmp(e, "0") != 0 && std::strcmp(e, "False") != 0 && std::strcmp(e, "false") != 0;
}
// Stream-level events instead of device-side polls (StageSync counters, gate / signal kernels): on request (RVIO_PARANOID), and when a
// counter-collecting profiler is attached (rocprofv3 --pmc exports ROCPROF_COUNTER_COLLECTION): it serialises kernels across queues, and a
// kernel that polls a counter another queue's kernel bumps would sit there until its 30 s time-out.
static bool no_device_polls() {
    static const bool v = (paranoid_bits() & PAR_NO_DEVPOLL) || profiler_serialises();
    return v;
}

// The dynamic-LDS limit of a kernel is a property of the PROCESS, not of a handle: a later handle with a smaller need (a shorter window, a
// smaller cornerSubPix half-window) must not lower it under an earlier live handle's launches — the limit only ever goes up.
static hipError_t lds_attr(const void* fn, int bytes) {
    static std::mutex mu;
    static std::map<const void*, int> limit;
    std::lock_guard<std::mutex> lk(mu);
    int& cur = limit[fn];
    if (bytes <= cur) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) cur = bytes;
    return e;
}
// launch_plan.h's kernels, in LpKernel order; its fixed sizes stand for these definitions
static_assert(LP_S9CHOL4_BYTES == sizeof(S9CholLds<4, 4>), "launch_plan.h: solve9's LDS structs");
static_assert(LP_S9CHOL6_BYTES == sizeof(S9CholLds<6, 4>), "launch_plan.h: solve9's LDS structs");
static_assert(LP_S9SMALL_BYTES == sizeof(S9SmallLds), "launch_plan.h: solve9's LDS structs");
static_assert(LP_PROP3_BYTES == sizeof(Prop3Lds<16>), "launch_plan.h: propagate's LDS struct");
static_assert(LP_JB_TL_DOUBLES == JB_TL_DOUBLES && LP_UGL_BYTES == UGL_LDS_DOUBLES * sizeof(double) && LP_FNL_BYTES == FNL_LDS_DOUBLES * sizeof(double) &&
              LP_JL_BYTES == JL_LDS_DOUBLES * sizeof(double), "launch_plan.h: the Joseph-form kernels' LDS");
static_assert(LP_DET_TW == DET_TW && LP_DET_FH == DET_FH && LP_DET_T == DET_T && LP_DET_SW == DET_SW && LP_DET_SH == DET_SH && LP_NEIGH_T == NEIGH_T &&
              LP_NEIGH_BLOCKS == NEIGH_BLOCKS && LP_NEIGH_BLOCKS_WIDE == NEIGH_BLOCKS_WIDE && LP_NEIGH_LDS == NEIGH_LDS && LP_GREEDY_T == GREEDY_T &&
              LP_GREEDY_LDS == GREEDY_LDS && LP_SP_WIN == SP_WIN && LP_SP_T == SP_T && LP_SPG_T == SPG_T && LP_SPW_C == SPW_C, "launch_plan.h: the detector's launch geometry");
static_assert(LP_PYR_T == PYR_T && LP_CLAHE_LUT_T == CLAHE_LUT_T, "launch_plan.h: pyramid / CLAHE workgroup sizes");
static const void* lp_kernel_fn(int k) {
    switch (k) {
        case LPK_FEAT_BUILD16: return (const void*)feat_build_kernel<16>;
        case LPK_FEAT_BUILD4: return (const void*)feat_build_kernel<4>;
        case LPK_GRAM_REDUCE: return (const void*)gram_reduce_kernel;
        case LPK_BLOCK_SUM: return (const void*)block_sum_kernel;
        case LPK_LIT_BATCH: return (const void*)lit_batch_kernel;
        case LPK_GEMM_T_LDS: return (const void*)gemm_T_lds_kernel;
        case LPK_GRAM_BATCH4: return (const void*)gram_reduce_batch_kernel<4>;
        case LPK_GRAM_BATCH6: return (const void*)gram_reduce_batch_kernel<6>;
        case LPK_FEAT_PROP: return (const void*)feat_prop_kernel;
        case LPK_BOOKKEEP_B: return (const void*)bookkeep_b_kernel;
        case LPK_RANSAC_BOOK: return (const void*)ransac_book_kernel;
        case LPK_SOLVE9_SMALL: return (const void*)solve9_small_kernel;
        case LPK_SOLVE6_1: return (const void*)solve6_kernel<1, 8, 8>;
        case LPK_SOLVE6_2: return (const void*)solve6_kernel<2, 12, 8>;
        case LPK_SOLVE6_3: return (const void*)solve6_kernel<2, 16, 8>;
        case LPK_JOSEPH_BATCH: return (const void*)joseph_batch_kernel;
        case LPK_UG: return (const void*)ug_kernel;
        case LPK_UG_LDS: return (const void*)ug_lds_kernel;
        case LPK_FINAL_LDS: return (const void*)final_lds_kernel;
        case LPK_JOSEPH_LDS: return (const void*)joseph_lds_kernel;
        case LPK_IMU_POSE: return (const void*)imu_pose_kernel;
        case LPK_AUX_UPDATE4: return (const void*)aux_update_kernel<4>;
        case LPK_AUX_UPDATE16: return (const void*)aux_update_kernel<16>;
        case LPK_IMU_COV: return (const void*)imu_cov_kernel;
        case LPK_STANDSTILL: return (const void*)standstill_kernel;
        case LPK_FIX: return (const void*)fix_rows_kernel;
        case LPK_FIX_PAST: return (const void*)fix_past_kernel;
        case LPK_REL: return (const void*)rel_rows_kernel;
        case LPK_MAP: return (const void*)map_rows_kernel;
        case LPK_AUX_ITER4: return (const void*)aux_iter_kernel<4>;
        case LPK_AUX_ITER16: return (const void*)aux_iter_kernel<16>;
        case LPK_WINDOW_POSE: return (const void*)window_pose_kernel;
        case LPK_WINDOW_EDGE: return (const void*)window_edge_kernel;
        case LPK_WINDOW_JOINT: return (const void*)window_joint_kernel;
        case LPK_LANDMARK_COV: return (const void*)landmark_cov_kernel;
    }
    return nullptr;
}
// static LDS of those kernels as the loaded code object has it (the compiler's decision: the plan budgets dynamic + static against a CU's 160 KiB)
static hipError_t static_lds_table(const size_t** out) {
    static std::mutex mu;
    static bool have = false;
    static size_t tab[LPK_COUNT];
    std::lock_guard<std::mutex> lk(mu);
    if (!have) {
        for (int k = 0; k < LPK_COUNT; ++k) {
            hipFuncAttributes a;
            const hipError_t e = hipFuncGetAttributes(&a, lp_kernel_fn(k));
            if (e != hipSuccess) return e;
            tab[k] = a.sharedSizeBytes;
        }
        have = true;
    }
    *out = tab;
    return hipSuccess;
}
static int create_impl(const rvio_config* cfg, int device, int batch, bool front_end, rvio_hip** out) {
    if (!cfg || !out) return RVIO_ERR_INVALID;
    *out = nullptr;
    if (cfg->max_track_len < 3 || cfg->max_track_len > RVIO_MAX_LEN || cfg->n_features < 2 || cfg->min_track_len < 2) return RVIO_ERR_INVALID;
    if (batch < 1) return RVIO_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return RVIO_ERR_NO_DEVICE;
    rvio_hip* h = new rvio_hip();
    h->cfg = *cfg; h->device = device; h->batch = batch;
    h->front_end = front_end; h->det_in_slab = front_end && batch > 1;
    h->wide_px = batch >= 8;   // (tests switch it through rvio_hip_debug_kernel_forms: the two forms must agree bit for bit)
    fill_devcfg(cfg, &h->dc);
    { rvio_calibration k; rvio_calibration_from_config(cfg, &k); h->cals.assign((size_t)batch, k); }
    const DevCfg& d = h->dc;
    h->img_cap = (size_t)d.W * d.H;
    if (d.grid_cols * d.grid_rows < 1) { delete h; return RVIO_ERR_INVALID; }
    *out = h;   // returned even on allocation failure so last_error is readable
    HIPCHK(h, hipSetDevice(device));
    // launch geometry (launch_plan.h: LDS sizes, kernel variants, what moves from LDS to global memory) — before anything is allocated: a configuration
    // whose footprint does not fit a CU beside the kernels' static LDS is refused here, not by a failed launch
    const size_t* statics = nullptr;
    HIPCHK(h, static_lds_table(&statics));
    h->plan = launch_plan(cfg->max_track_len, cfg->n_features, batch, statics);
    const LaunchPlan& plan = h->plan;
    if (plan.rc) { h->err = plan.why; return RVIO_ERR_UNSUPPORTED; }
    h->private_queues = g_private_queue_handles.fetch_add(1) == 0;
    if (!h->private_queues) g_private_queue_handles.fetch_sub(1);
    HIPCHK(h, make_stream(h, &h->stream));
    HIPCHK(h, make_stream(h, &h->stream_t));
    HIPCHK(h, make_stream(h, &h->stream_d));
    HIPCHK(h, make_stream(h, &h->stream_c));
    // Image chains in flight (plan.n_ic).  Two (default): with the filter, tracker and side streams that makes FOUR busy queues.  A third chain on a
    // fifth queue was measured: the frame period goes from 131 to 180-250 us whatever CUs the front end is kept off — beyond
    // four busy queues the command processor time-slices them.
    // Long windows (96 < 6n <= 192: the solve in its split form, filter chain >= 250 us): ONE image chain in flight is enough (the chain is ~180 us),
    // and the queue that frees runs the Cholesky factor of the clone block beside the filter chain (augment_compose_dev).  A FIFTH queue for it was
    // measured: cfg C 3.2 k frames/s instead of 3.9 k — the command processor time-slices beyond four busy queues.
    if (plan.chol_queue) {
        h->stream_l = h->stream_c;
        RCCHK(own_event(h, &h->evA, kEvFlags));
        RCCHK(own_event(h, &h->evL, kEvFlags));
    }
    RCCHK(own_event(h, &h->evD0, kEvFlags));
    RCCHK(own_event(h, &h->evD1, kEvFlags));
    for (int b = 0; b < rvio_hip::kIC; ++b) RCCHK(own_event(h, &h->evC[b], kEvFlags));
    for (int b = 0; b < 2; ++b) {
        RCCHK(own_event(h, &h->evT[b], kEvFlags));
        RCCHK(own_event(h, &h->evT[b + 2], kEvFlags));
        RCCHK(own_event(h, &h->evH[b], kEvFlags));
        RCCHK(own_event(h, &h->evH[b + 2], kEvFlags));
        RCCHK(own_event(h, &h->evF[b], kEvFlags));
        RCCHK(own_event(h, &h->evF[b + 2], kEvFlags));
        RCCHK(own_event(h, &h->evIn[b], kEvFlags));
    }
    if (front_end && cfg->enable_equalizer) {   // CLAHE(3.0, 5x5), Tracker.cc:198-202
        h->cl_tx = 5; h->cl_ty = 5;
        int ew = d.W, eh = d.H;
        if (d.W % h->cl_tx != 0 || d.H % h->cl_ty != 0) { ew = d.W + (h->cl_tx - d.W % h->cl_tx); eh = d.H + (h->cl_ty - d.H % h->cl_ty); }
        h->cl_tw = ew / h->cl_tx; h->cl_th = eh / h->cl_ty;
        const int area = h->cl_tw * h->cl_th;
        h->cl_clip = std::max((int)(3.0 * area / 256), 1);
        h->cl_scale = 255.0f / (float)area;
    }
    if (h->det_in_slab) { int rc = detector_check(h); if (rc != RVIO_OK) return rc; }
    // instance slab(s)
    h->slab_mode = true; h->slab = nullptr; h->slab_off = 0;
    { int rc = alloc_filter_slab(h); if (rc != RVIO_OK) return rc; }
    if (front_end) { int rc = alloc_frontend_slab(h); if (rc != RVIO_OK) return rc; }
    h->slab_bytes = h->slab_off;
    {
        RCCHK(own_dev(h, &h->slab, h->slab_bytes * (size_t)batch, true));
        h->slab_off = 0;
    }
    { int rc = alloc_filter_slab(h); if (rc != RVIO_OK) return rc; }
    if (front_end) { int rc = alloc_frontend_slab(h); if (rc != RVIO_OK) return rc; }
    h->slab_mode = false;
    h->bin = {0, h->slab_bytes, h->slab_bytes, h->slab_bytes, h->slab_bytes};
    TrackerDev& t = h->t;
    t.info = h->d_info;
    t.first_host = nullptr;
    if (front_end) {
        RCCHK(own_pinned(h, &h->first_mirror, sizeof(int) * (size_t)batch, hipHostMallocMapped));
        for (int i = 0; i < batch; ++i) h->first_mirror[i] = 1;
        void* dp_ = nullptr;
        HIPCHK(h, hipHostGetDevicePointer(&dp_, h->first_mirror, 0));
        t.first_host = (int*)dp_;
    }
    h->tout[0] = {t.n_feat, t.types, t.len, t.meas};   // Tracker -> Updater hand-over, double-buffered for the pipelined path
    if (front_end) {   // mbIsTheFirstImage = true in every instance
        std::vector<int> ones((size_t)batch, 1);
        HIPCHK(h, hipMemcpy2DAsync(t.first, h->slab_bytes, ones.data(), sizeof(int), sizeof(int), (size_t)batch, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (plan.solve9_nt) DALLOC(h, h->S9scr, S9_SLAB_DOUBLES(plan.solve9_nt) * (size_t)batch);
    for (int k = 0; k < LPK_COUNT; ++k)
        if (plan.attr[k]) HIPCHK(h, lds_attr(lp_kernel_fn(k), (int)plan.attr[k]));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}

int rvio_hip_create(const rvio_config* cfg, int device, rvio_hip** out) { return create_impl(cfg, device, 1, true, out); }
// B independent instances behind one handle: every stage is ONE launch with gridDim.z = B.
// front_end = 0: filter only (rvio_hip_frame_tracks_dev); 1: with CLAHE / detector / KLT / RANSAC / book-keeping (rvio_hip_frame_batch_dev)
int rvio_hip_create_batch(const rvio_config* cfg, int device, int n_instances, int front_end, rvio_hip** out) {
    return create_impl(cfg, device, n_instances, front_end != 0, out);
}
int rvio_hip_batch_size(const rvio_hip* h) { return h ? h->batch : 0; }

void rvio_hip_destroy(rvio_hip* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream_c) hipStreamSynchronize(h->stream_c);
    if (h->stream_d) hipStreamSynchronize(h->stream_d);
    if (h->stream_t) hipStreamSynchronize(h->stream_t);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->private_queues) g_private_queue_handles.fetch_sub(1);
    for (const rvio_hip::Owned& o : h->owned) own_free(o);   // the slab, every event, everything allocated on demand (the streams are idle)
    if (h->stream_d) hipStreamDestroy(h->stream_d);
    if (h->stream_c) hipStreamDestroy(h->stream_c);
    if (h->stream_t) hipStreamDestroy(h->stream_t);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}
const char* rvio_hip_last_error(const rvio_hip* h) { return h ? h->err.c_str() : "null handle"; }
void* rvio_hip_stream(rvio_hip* h) { return h ? (void*)h->stream : nullptr; }
// every stream of the handle, nothing else (no error check: the recovery paths use it)
static int drain_all(rvio_hip* h) {
    HIPCHK(h, hipSetDevice(h->device));
    SYNC_FRONT(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}
// (Read-backs go through the handle's own stream: the CU-mask streams of the first live handle are created by
// hipExtStreamCreateWithCUMask as BLOCKING streams, a later handle's as non-blocking ones — a NULL-stream hipMemcpy would synchronise with
// the former only, and with whatever else the process has on its NULL stream.)
int rvio_hip_sync(rvio_hip* h) {
    if (!h) return RVIO_ERR_INVALID;
    { const int rc = drain_all(h); if (rc != RVIO_OK) return rc; }
    // a device-side stage counter that timed out (stage_wait, rvio_dev.h) left the frame sequence broken: a hard error, not a flag to poll.
    // rvio_hip_initialize is the way out of it (it resets the counters and clears the flag).
    int e = 0;
    HIPCHK(h, hipMemcpyAsync(&e, &h->meta->err, sizeof e, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (e & 4) { h->err = "a device-side stage counter timed out (filter -> book-keeping): the frame sequence is invalid, re-initialise"; return RVIO_ERR_STATE; }
    return RVIO_OK;
}

// ------------------------------------------------------------------ the cached factor of the clone block
// solve9 can start from a Cholesky factor of P's clone block that was computed ahead of the solve and lies in the solve9 slab (S9scr):
//   chol_ready   a role workgroup of a launch already on the filter stream writes it (6n <= 96): stream order puts it in front of the solve
//   chol_async   it was queued on stream_l behind augment/compose (6n > 96) and evL is recorded behind it: the solve waits for evL
// THE RULE: whoever writes P's clone block in place (anything but propagate, which leaves that block alone), replaces P, or rewrites the
// slab calls chol_drop() in front of the write — or the next solve at 6n > 96 starts from the factor of another matrix, silently.  chol_drop
// says how a factor still in flight on stream_l is awaited, because it READS the covariance that is about to change.
// No other code touches the two flags.
static void chol_role(rvio_hip* h, bool writes) { h->chol_ready = writes; }   // the launch just enqueued: its role workgroup writes the factor (false: it has none)
static void chol_queued(rvio_hip* h) { h->chol_async = true; }                // the factor was just enqueued on stream_l, evL behind it
//   CHOL_FILTER_WAITS   the writer is enqueued on the filter stream: that stream waits for evL
//   CHOL_HOST_WAITS     the writer runs on the host's schedule: the host waits for stream_l
//   CHOL_DRAINED        the caller has drained every stream of the handle
enum CholAwait { CHOL_FILTER_WAITS, CHOL_HOST_WAITS, CHOL_DRAINED };
static int chol_drop(rvio_hip* h, CholAwait how) {
    if (h->chol_async) {
        if (how == CHOL_FILTER_WAITS) HIPCHK(h, hipStreamWaitEvent(h->stream, h->evL, 0));
        else if (how == CHOL_HOST_WAITS) HIPCHK(h, hipStreamSynchronize(h->stream_l));
        h->chol_async = false;
    }
    h->chol_ready = false;
    return RVIO_OK;
}
// Take it for the solve: is a factor of the clone block in the slab, or about to be (stream_l: the solve waits for it; a failed wait: the
// solve factors Pcc itself)?  The solve behind this call consumes it.
static bool take_chol(rvio_hip* h) {
    if (h->chol_async && hipStreamWaitEvent(h->stream, h->evL, 0) != hipSuccess) { h->chol_async = false; h->chol_ready = false; }
    const bool pre = h->chol_ready || h->chol_async;
    h->chol_ready = false; h->chol_async = false;
    return pre;
}

// ------------------------------------------------------------------ state
static int set_state_range(rvio_hip* h, int lo, int hi, const double* x, int xdim, const double* P, int d) {
    if (!h || !x || !P) return RVIO_ERR_INVALID;
    const int n = (xdim - 26) / 7;
    if (xdim != 26 + 7 * n || d != 24 + 6 * n || n < 0 || n > h->dc.nmax) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    FilterMeta m; std::memset(&m, 0, sizeof m);
    m.n_clones = n; m.img_count = h->img_count;
    RCCHK(chol_drop(h, CHOL_HOST_WAITS));   // (the covariance is about to be replaced)
    for (int i = lo; i < hi; ++i) {
        const size_t o = (size_t)i * h->slab_bytes;
        double* Pi = (double*)((char*)h->P[h->cur] + o);
        HIPCHK(h, hipMemsetAsync(Pi, 0, sizeof(double) * h->dc.dmax * h->dc.dmax, h->stream));
        HIPCHK(h, hipMemcpyAsync((char*)h->x[h->cur] + o, x, sizeof(double) * xdim, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpy2DAsync(Pi, sizeof(double) * h->dc.dmax, P, sizeof(double) * d, sizeof(double) * d, d, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync((char*)h->meta + o, &m, sizeof m, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_clones_host = n;
    h->composed_count = h->img_count;   // (a state handed in is a composed one: its newest clone ends at its reference frame)
    h->has_state = true;
    return RVIO_OK;
}
// (a batch handle: every instance receives the same state)
int rvio_hip_set_state(rvio_hip* h, const double* x, int xdim, const double* P, int d) { return h ? set_state_range(h, 0, h->batch, x, xdim, P, d) : RVIO_ERR_INVALID; }
// one instance of a batch handle; the window length is common to all instances (it depends on the frame count only)
int rvio_hip_set_state_at(rvio_hip* h, int instance, const double* x, int xdim, const double* P, int d) {
    if (!h || instance < 0 || instance >= h->batch || xdim != 26 + 7 * h->n_clones_host) return RVIO_ERR_INVALID;
    return set_state_range(h, instance, instance + 1, x, xdim, P, d);
}

int rvio_hip_get_state_at(rvio_hip* h, int instance, double* x, int* xdim, double* P, int* d) {
    if (!h || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t o = (size_t)instance * h->slab_bytes;
    const int n = h->n_clones_host, dd = 24 + 6 * n, xd = 26 + 7 * n;
    if (xdim) *xdim = xd;
    if (d) *d = dd;
    if (x) HIPCHK(h, hipMemcpyAsync(x, (char*)h->x[h->cur] + o, sizeof(double) * xd, hipMemcpyDeviceToHost, h->stream));
    if (P) HIPCHK(h, hipMemcpy2DAsync(P, sizeof(double) * dd, (char*)h->P[h->cur] + o, sizeof(double) * h->dc.dmax, sizeof(double) * dd, dd,
                                      hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}
int rvio_hip_get_state(rvio_hip* h, double* x, int* xdim, double* P, int* d) { return rvio_hip_get_state_at(h, 0, x, xdim, P, d); }

// System::initialize (System.cc:115-170) on the host: the gravity-aligned x(26) and the diagonal P(24 x 24) of one filter
static void initial_state(const rvio_config& c, const double w[3], const double a[3], int n_imu, double x[26], double P[576]) {
    double an = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    double g[3] = {a[0] / an, a[1] / an, a[2] / an};
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (c.ini_enable_alignment) {
        double xv[3], yv[3];
        const double ex[3] = {1, 0, 0};
        for (int i = 0; i < 3; ++i) xv[i] = ex[i] - (g[i] * g[0] * ex[0] + g[i] * g[1] * ex[1] + g[i] * g[2] * ex[2]);
        double xn = std::sqrt(xv[0] * xv[0] + xv[1] * xv[1] + xv[2] * xv[2]);
        for (int i = 0; i < 3; ++i) xv[i] /= xn;
        yv[0] = -g[2] * xv[1] + g[1] * xv[2]; yv[1] = g[2] * xv[0] - g[0] * xv[2]; yv[2] = -g[1] * xv[0] + g[0] * xv[1];
        double yn = std::sqrt(yv[0] * yv[0] + yv[1] * yv[1] + yv[2] * yv[2]);
        for (int i = 0; i < 3; ++i) yv[i] /= yn;
        for (int i = 0; i < 3; ++i) { R[3 * i] = xv[i]; R[3 * i + 1] = yv[i]; R[3 * i + 2] = g[i]; }
    }
    // RotToQuat (Numerics.h:126-167), host copy
    double q[4]; const double T = R[0] + R[4] + R[8];
    if (R[0] > T && R[0] > R[4] && R[0] > R[8]) { q[0] = std::sqrt((1 + 2 * R[0] - T) / 4); double k = 1 / (4 * q[0]); q[1] = k * (R[1] + R[3]); q[2] = k * (R[2] + R[6]); q[3] = k * (R[5] - R[7]); }
    else if (R[4] > T && R[4] > R[0] && R[4] > R[8]) { q[1] = std::sqrt((1 + 2 * R[4] - T) / 4); double k = 1 / (4 * q[1]); q[0] = k * (R[1] + R[3]); q[2] = k * (R[5] + R[7]); q[3] = k * (R[6] - R[2]); }
    else if (R[8] > T && R[8] > R[0] && R[8] > R[4]) { q[2] = std::sqrt((1 + 2 * R[8] - T) / 4); double k = 1 / (4 * q[2]); q[0] = k * (R[2] + R[6]); q[1] = k * (R[5] + R[7]); q[3] = k * (R[1] - R[3]); }
    else { q[3] = std::sqrt((1 + T) / 4); double k = 1 / (4 * q[3]); q[0] = k * (R[5] - R[7]); q[1] = k * (R[6] - R[2]); q[2] = k * (R[1] - R[3]); }
    double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] /= qn;
    if (q[3] < 0) for (int i = 0; i < 4; ++i) q[i] = -q[i];
    std::memset(x, 0, sizeof(double) * 26); std::memset(P, 0, sizeof(double) * 576);
    for (int i = 0; i < 4; ++i) x[i] = q[i];
    for (int i = 0; i < 3; ++i) x[7 + i] = g[i];
    if (n_imu > 1) for (int i = 0; i < 3; ++i) { x[20 + i] = w[i]; x[23 + i] = a[i] - c.gravity * g[i]; }
    const double dt = 1. / c.imu_rate;
    auto D = [&](int i, double v) { P[i * 24 + i] = v; };
    for (int i = 0; i < 6; ++i) D(i, std::pow(1e-3, 2));
    for (int i = 6; i < 9; ++i) D(i, n_imu * dt * std::pow(c.sigma_a, 2));
    for (int i = 18; i < 21; ++i) D(i, n_imu * dt * std::pow(c.sigma_wg, 2));
    for (int i = 21; i < 24; ++i) D(i, n_imu * dt * std::pow(c.sigma_wa, 2));
}
// ... runs once; result uploaded to every instance, and the handle starts over (frame count, tracker, cloud, odometry ring).  Calibrations stay.
int rvio_hip_initialize(rvio_hip* h, const double w[3], const double a[3], int n_imu) {
    if (!h || !w || !a) return RVIO_ERR_INVALID;
    double x[26], P[576];
    initial_state(h->cfg, w, a, n_imu, x, P);
    h->img_count = 0;
    h->lm_frame = -1;   // no cloud since initialisation (the enable flag stays)
    h->lmc_frame = -1;
    h->odom.seq = 0;    // ... and no odometry record: seq restarts at 1 (the getters read nothing beyond seq)
    h->smo.seq = 0;     // ... nor a smoothed one
    h->edg.seq = 0;     // ... nor an edge
    h->imuo.seq = 0;    // ... nor an IMU-rate record
    h->imuc.seq = 0; h->imuc_first = 1;   // ... nor its covariance
    // a (re-)initialised filter starts with an empty window: the tracker starts over too (mbIsTheFirstImage, Tracker.cc:88), or its
    // histories would be longer than the window they refer to
    if (h->front_end) {
        // (plain drains, not rvio_hip_sync: re-initialising is the recovery path after a stage counter timed out — RVIO_ERR_STATE —, so the
        // sticky flag must not keep the handle from getting here; set_state below rewrites FilterMeta, flag included)
        int rc0 = drain_all(h);
        if (rc0 != RVIO_OK) return rc0;
        // the device-side counters start over together with their host-side targets: after a time-out they no longer agree
        HIPCHK(h, hipMemsetAsync(h->stage_sync, 0, sizeof(StageSync), h->stream));
        h->stage_tgt = StageSync{};
        for (int b = 0; b < rvio_hip::kHand; ++b) { h->fin_mode[b] = 0; h->fin_target[b] = 0; }
        h->last_ra = false;
        std::vector<int> ones((size_t)h->batch, 1);
        HIPCHK(h, hipMemcpy2DAsync(h->t.first, h->slab_bytes, ones.data(), sizeof(int), sizeof(int), (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
        for (int i = 0; i < h->batch; ++i) {
            const size_t o = (size_t)i * h->slab_bytes;
            HIPCHK(h, hipMemsetAsync((char*)h->t.n_pts + o, 0, sizeof(int), h->stream));
            HIPCHK(h, hipMemsetAsync((char*)h->t.hist_len + o, 0, sizeof(int) * h->dc.F, h->stream));
            for (int b = 0; b < rvio_hip::kHand; ++b) HIPCHK(h, hipMemsetAsync((char*)h->tout[b].n_feat + o, 0, sizeof(int), h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->frame_no = 0; h->piped = false; h->in_frame = false; h->fuse_m = -1;
        for (int i = 0; i < h->batch; ++i) h->first_mirror[i] = 1;
        h->first_cleared = false;
    }
    return rvio_hip_set_state(h, x, 26, P, 24);
}
// The same state for ONE instance (each robot of a fleet has its own gravity direction and biases), stored as rvio_hip_set_state_at stores it:
// none of the handle-wide resets above, so it belongs in front of the first frame — the window must be empty
int rvio_hip_initialize_at(rvio_hip* h, int instance, const double w[3], const double a[3], int n_imu) {
    if (!h || !w || !a || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    if (h->n_clones_host != 0) { h->err = "rvio_hip_initialize_at needs an empty window (call it before the first frame)"; return RVIO_ERR_STATE; }
    double x[26], P[576];
    initial_state(h->cfg, w, a, n_imu, x, P);
    return set_state_range(h, instance, instance + 1, x, 26, P, 24);
}

// ------------------------------------------------------------------ per-instance calibration
static bool calibration_ok(const rvio_calibration* c) {
    const float f[9] = {c->fx, c->fy, c->cx, c->cy, c->k1, c->k2, c->p1, c->p2, c->k3};
    for (float v : f) if (!std::isfinite(v)) return false;
    for (double v : c->T_bc) if (!std::isfinite(v)) return false;
    return c->fx != 0.f && c->fy != 0.f;
}
// entries [lo, hi) become src[0 .. hi - lo): drain the handle (like rvio_hip_set_image_format: nothing in flight reads the table), allocate the
// table on first use — every instance starts from the config's calibration — and upload what changed
static int set_calibration_range(rvio_hip* h, int lo, int hi, const rvio_calibration* src) {
    for (int i = lo; i < hi; ++i)
        if (!calibration_ok(src + (i - lo))) { h->err = "calibration of instance " + std::to_string(i) + ": a non-finite member, or fx / fy = 0"; return RVIO_ERR_INVALID; }
    { const int rc = drain_all(h); if (rc != RVIO_OK) return rc; }
    const bool fresh = !h->cal;
    if (fresh) RCCHK(own_dev(h, &h->cal, sizeof(CamCal) * (size_t)h->batch));
    for (int i = lo; i < hi; ++i) h->cals[(size_t)i] = src[i - lo];
    const int first = fresh ? 0 : lo, last = fresh ? h->batch : hi;
    std::vector<CamCal> dev((size_t)(last - first));
    for (int i = first; i < last; ++i) fill_camcal(&h->cals[(size_t)i], &dev[(size_t)(i - first)]);
    HIPCHK(h, hipMemcpyAsync(h->cal + first, dev.data(), sizeof(CamCal) * dev.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (`dev` is a stack-lifetime staging buffer)
    return RVIO_OK;
}
int rvio_hip_set_calibration_at(rvio_hip* h, int instance, const rvio_calibration* c) {
    if (!h || !c || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    return set_calibration_range(h, instance, instance + 1, c);
}
int rvio_hip_set_calibrations(rvio_hip* h, const rvio_calibration* all) {
    if (!h || !all) return RVIO_ERR_INVALID;
    return set_calibration_range(h, 0, h->batch, all);
}
int rvio_hip_get_calibration_at(rvio_hip* h, int instance, rvio_calibration* c) {
    if (!h || !c || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    *c = h->cals[(size_t)instance];
    return RVIO_OK;
}

// ------------------------------------------------------------------ P1
// PreIntegrator::propagate iterates whatever list it is handed (PreIntegrator.cc:96-97) — a dropped image or a stalled camera driver makes
// that list long.  The kernels take any m (propagate and RANSAC's gyro prior walk the samples in chunks); what is sized is the staging of
// the HOST-buffer entry points: RVIO_HIP_MAX_IMU samples are allocated up front, a longer batch grows it once (the host waits for the
// handle's streams, allocates, goes on) instead of being refused.
// the pinned ring of rvio_hip_frame is laid out for one image size and IMU capacity: when either changes (on a drained handle) its blocks go,
// and the next rvio_hip_frame allocates them again (the events stay)
static void drop_pin_ring(rvio_hip* h) {
    for (int k = 0; k < rvio_hip::kPin; ++k) { own_release(h, h->pin[k]); h->pin[k] = nullptr; }
}
static int ensure_imu_capacity(rvio_hip* h, int m) {
    if (m <= h->imu_cap) return RVIO_OK;
    int rc = drain_all(h);   // (an earlier device-side error stays visible through rvio_hip_sync / rvio_hip_get_frame_info)
    if (rc != RVIO_OK) return rc;
    const int cap = std::max(2 * h->imu_cap, (m + 63) & ~63);
    // (the old block stays where it was — a slab member, or a block freed with the handle)
    auto grow = [&](rvio_imu** p) { return own_dev(h, p, sizeof(rvio_imu) * (size_t)cap); };
    if ((rc = grow(&h->d_imu)) != RVIO_OK) return rc;
    for (int k = 0; k <= rvio_hip::kHand; ++k) if (h->hb_imu[k] && (rc = grow(&h->hb_imu[k])) != RVIO_OK) return rc;
    drop_pin_ring(h);   // rvio_hip_frame lays the ring out again
    h->imu_cap = cap;
    return RVIO_OK;
}
// the forms of an update at clone count n (launch_plan.h update_forms): every launch function below takes its decisions from here
static UpdateForms forms_at(const rvio_hip* h, int n, bool pre = false, bool whole_update = true, bool combined = true) {
    return update_forms(h->plan, h->batch, n, pre, whole_update, combined, h->lit_rows != nullptr);
}
// imu_pose_kernel (imu_pose.hip) on `instances` instances whose state starts at x: records of d_imu[0 .. m) from that state.  cap == 0: into
// out[z * out_stride + j] (rvio_hip_predict*); cap > 0: into the ring `out`, record j with seq = seq0 + j
static void launch_imu_pose(rvio_hip* h, hipStream_t st, int instances, const double* x, const rvio_imu* d_imu, size_t imu_bs, int m, rvio_imu_pose* out,
                            long long out_stride, long long seq0, int cap, int img_count) {
    const LpLaunch l = imu_pose_launch(instances);
    hipLaunchKernelGGL(imu_pose_kernel, dim3((unsigned)l.gx), dim3((unsigned)l.threads), l.lds, st, h->dc.small_angle, h->dc.gravity, instances, x, h->slab_bytes, d_imu, imu_bs, m,
                       (unsigned long long*)out, out_stride, seq0, cap, img_count);
}
// imu_cov_kernel (imu_cov.hip) beside it: the same operands plus the 24 x 24 head of P, the same addressing of `out`
static void launch_imu_cov(rvio_hip* h, hipStream_t st, int instances, const double* x, const double* P, const rvio_imu* d_imu, size_t imu_bs, int m, rvio_imu_cov* out,
                           long long out_stride, long long seq0, int cap, int img_count) {
    const LpLaunch l = imu_cov_launch(instances);
    hipLaunchKernelGGL(imu_cov_kernel, dim3((unsigned)l.gx), dim3((unsigned)l.threads), l.lds, st, h->dc.small_angle, h->dc.gravity, h->dc.sg2, h->dc.swg2, h->dc.sa2, h->dc.swa2, instances, x, P,
                       h->dc.dmax, h->slab_bytes, d_imu, imu_bs, m, (unsigned long long*)out, out_stride, seq0, cap, img_count);
}
// The IMU-rate ring's launch: directly in front of whatever propagates in place, on the stream that propagate runs on (it reads the state that
// propagate is about to overwrite, and the same samples).  img_count: nImageCountAfterInit of the frame that consumes the samples.
static int imu_ring_record(rvio_hip* h, const rvio_imu* d_imu, int m, size_t imu_bs, hipStream_t st, int img_count) {
    if (!h->imuo.on || m <= 0) return RVIO_OK;
    launch_imu_pose(h, st, h->batch, h->x[h->cur], d_imu, imu_bs, m, h->imuo.ring, 0, h->imuo.seq + 1, h->imuo.cap, img_count);
    HIPCHK(h, hipGetLastError());
    if (h->imuc.on) {   // the covariance records of the same samples: same seq, same slots
        launch_imu_cov(h, st, h->batch, h->x[h->cur], h->P[h->cur], d_imu, imu_bs, m, h->imuc.ring, 0, h->imuo.seq + 1, h->imuo.cap, img_count);
        HIPCHK(h, hipGetLastError());
        h->imuc.seq = h->imuo.seq + m;
    }
    h->imuo.seq += m;   // (counted once the launch is known to be enqueued: the getter serves nothing beyond seq)
    return RVIO_OK;
}
// img_count: nImageCountAfterInit of the frame this propagate belongs to, for the IMU-rate ring's records (-1: the handle's current count — every caller
// that has advanced it already; the pipelined frame propagates ahead of frame_tail_dev's increment and passes the next count)
static int propagate_dev(rvio_hip* h, const rvio_imu* d_imu, int m, size_t imu_bs = 0, hipStream_t st = nullptr, int img_count = -1) {   // imu_bs = 0: every instance integrates the same samples
    if (!st) st = h->stream;
    h->time_imu = d_imu; h->time_m = m; h->time_imu_bs = imu_bs;   // (rvio_hip_debug_time_kernel(8), (13))
    if (h->imuo.on) { const int rci = imu_ring_record(h, d_imu, m, imu_bs, st, img_count < 0 ? h->img_count : img_count); if (rci != RVIO_OK) return rci; }
    if (h->batch > 8)
        hipLaunchKernelGGL(propagate_kernel3b, dim3(1, 1, h->batch), dim3(256), 0, st, h->dc, h->meta, h->n_clones_host, h->x[h->cur], h->P[h->cur], d_imu, m,
                           h->slab_bytes, imu_bs);
    else if (forms_at(h, h->n_clones_host).chol == LPC_ROLE && !imu_bs) {
        // plain handle, 6n <= 96: the Cholesky role of the solve (solve9.hip) as a second workgroup — the clone block it factors is the one the update
        // behind this propagate will see (propagation does not touch it)
        const int nc = h->n_clones_host;
        if (h->plan.solve9_nt == 4) hipLaunchKernelGGL(propagate_chol_kernel<2>, dim3(2), dim3(256), 0, st, h->dc, h->meta, nc, h->x[h->cur], h->P[h->cur], d_imu, m, h->S9scr);
        else hipLaunchKernelGGL(propagate_chol_kernel<3>, dim3(2), dim3(256), 0, st, h->dc, h->meta, nc, h->x[h->cur], h->P[h->cur], d_imu, m, h->S9scr);
        chol_role(h, true);
    }
    else
    hipLaunchKernelGGL(propagate_kernel3, dim3(1, 1, h->batch), dim3(256), 0, st, h->dc, h->meta, h->n_clones_host, h->x[h->cur], h->P[h->cur], d_imu, m,
                       h->slab_bytes, imu_bs);
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}
int rvio_hip_propagate(rvio_hip* h, const rvio_imu* imu, int m) {
    if (!h || (!imu && m > 0) || m < 0) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    { const int rcg = ensure_imu_capacity(h, m); if (rcg != RVIO_OK) return rcg; }
    if (m > 0) HIPCHK(h, hipMemcpyAsync(h->d_imu, imu, sizeof(rvio_imu) * m, hipMemcpyHostToDevice, h->stream));
    return propagate_dev(h, h->d_imu, m);
}

// ------------------------------------------------------------------ U1..U10
static int upload_tracks(rvio_hip* h, const rvio_tracks* tr) {
    const DevCfg& d = h->dc;
    if (!tr || tr->n_feat < 0 || tr->n_feat > d.Fu) return RVIO_ERR_INVALID;
    std::vector<float> meas((size_t)d.Fu * d.max_len * 2, 0.f);
    for (int f = 0; f < tr->n_feat; ++f) {
        if (tr->len[f] < 2 || tr->len[f] > d.max_len || tr->len[f] > tr->max_len) return RVIO_ERR_INVALID;
        if (tr->len[f] - 1 > h->n_clones_host) return RVIO_ERR_INVALID;
        std::memcpy(&meas[(size_t)f * d.max_len * 2], tr->meas + (size_t)f * tr->max_len * 2, sizeof(float) * 2 * tr->len[f]);
    }
    int nf = tr->n_feat;
    HIPCHK(h, hipMemcpyAsync(h->t.n_feat, &nf, sizeof nf, hipMemcpyHostToDevice, h->stream));
    if (nf > 0) {
        HIPCHK(h, hipMemcpyAsync(h->t.types, tr->types, nf, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->t.len, tr->len, sizeof(int) * nf, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->t.meas, meas.data(), sizeof(float) * meas.size(), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));   // `meas` is a stack-lifetime staging buffer
    return RVIO_OK;
}

static LitArgs lit_args(const rvio_hip* h, size_t lds_bytes) { return LitArgs{h->lit_rows, h->lit_rows ? h->lit_state : nullptr, h->t.n_feat, lds_bytes / sizeof(double)}; }
// U1..U5 of shard `rank` of `world`, one workgroup per feature slot: the latency form for one stream (every operand load of a gate tile in flight at
// once), the throughput form for a batch (with geom4_kernel's pose chains where the handle has them)
static void launch_feat_build(rvio_hip* h, int n, int rank, int world) {
    const DevCfg& d = h->dc;
    const dim3 g(d.Fu, 1, h->batch), b(h->plan.feat_threads);
    if (h->batch == 1)
        hipLaunchKernelGGL(feat_build_kernel<16>, g, b, h->plan.feat_lds, h->stream, d, n, h->x[h->cur], h->P[h->cur],
                           h->t.n_feat, h->t.types, h->t.len, h->t.meas, rank, world, h->partial, h->nrows, h->acc, h->ndof, h->gamma, h->pfinv,
                           h->tm_global, h->slab_bytes, h->bin, h->meta, (const double*)nullptr, (const int*)nullptr, h->lit_rows, (const CamCal*)h->cal);
    else
        hipLaunchKernelGGL(feat_build_kernel<4>, g, b, h->plan.feat_lds, h->stream, d, n, h->x[h->cur], h->P[h->cur],
                           h->t.n_feat, h->t.types, h->t.len, h->t.meas, rank, world, h->partial, h->nrows, h->acc, h->ndof, h->gamma, h->pfinv,
                           h->tm_global, h->slab_bytes, h->bin, h->meta, (const double*)h->gpose, (const int*)h->gvalid, h->lit_rows, (const CamCal*)h->cal);
}
// propagate + U1..U5 in one launch (independent: see feat_prop_kernel); single instance (sharded or not: every rank propagates, builds its features)
static void launch_feat_prop(rvio_hip* h, int n, const rvio_imu* d_imu, int m, int rank, int world) {
    const DevCfg& d = h->dc;
    // solve9 at 6n <= 96: the Cholesky of the clone block as one more workgroup of this launch (the solve of this very update follows on the stream)
    const bool chol = forms_at(h, n).chol == LPC_ROLE;
    hipLaunchKernelGGL(feat_prop_kernel, dim3(d.Fu + 1 + (chol ? 1 : 0)), dim3(256), h->plan.fprop_lds, h->stream, d, n, h->x[h->cur], h->P[h->cur],
                       h->t.n_feat, h->t.types, h->t.len, h->t.meas, h->partial, h->nrows, h->acc, h->ndof, h->gamma, h->pfinv, h->tm_global, h->bin,
                       h->meta, d_imu, m, chol ? h->S9scr : (double*)nullptr, h->plan.solve9_nt, rank, world, h->lit_rows, (const CamCal*)h->cal);
    chol_role(h, chol);
}
// reduction of the per-feature shares into [S2 | S1]; gram_finish: the last workgroup turns the block into [A|b] in place (rank truncation included), as the
// batch kernels always do — behind them the literal sweep for the instances whose small stacks need it (literal.h)
static void launch_gram(rvio_hip* h, const UpdateForms& f, int n) {
    const DevCfg& d = h->dc;
    const int B = h->batch;
    const dim3 g(f.gram_grid, 1, B), b(256);
    switch (f.gram) {
    case LPG_REDUCE:
        hipLaunchKernelGGL(gram_reduce_kernel, g, b, f.gram_lds.bytes, h->stream, d, n, h->partial, h->nrows, h->t.types, h->t.len, h->block, h->gram_cnt,
                           f.gram_finish ? 1 : 0, (B == 1) ? 1 : 0, h->slab_bytes, h->bin, lit_args(h, f.gram_lds.bytes));
        break;
    case LPG_BATCH4: hipLaunchKernelGGL(gram_reduce_batch_kernel<4>, g, b, f.gram_lds.bytes, h->stream, d, n, h->partial, h->nrows, h->t.types, h->t.len, h->block, h->slab_bytes, h->bin); break;
    case LPG_BATCH6: hipLaunchKernelGGL(gram_reduce_batch_kernel<6>, g, b, f.gram_lds.bytes, h->stream, d, n, h->partial, h->nrows, h->t.types, h->t.len, h->block, h->slab_bytes, h->bin); break;
    }
    if (f.lit_batch)
        hipLaunchKernelGGL(lit_batch_kernel, g, b, f.lit_lds.bytes, h->stream, d, n, (const int*)h->nrows,
                           (const unsigned char*)h->t.types, (const int*)h->t.len, h->block, h->slab_bytes, h->bin, lit_args(h, f.lit_lds.bytes));
}

static int update_local_dev(rvio_hip* h, int rank, int world, bool combine) {
    const DevCfg& d = h->dc;
    const int n = h->n_clones_host;
    const int B = h->batch;
    if (h->fuse_m >= 0) {
        // (the frame count is this frame's: frame_tail_dev / the sharded frame have advanced it)
        if (h->imuo.on) { const int rci = imu_ring_record(h, h->fuse_imu, h->fuse_m, 0, h->stream, h->img_count); if (rci != RVIO_OK) return rci; }
        launch_feat_prop(h, n, h->fuse_imu, h->fuse_m, rank, world);
        h->fuse_m = -1;
    } else {
        if (h->gpose)   // U1 + U2 four features per wave, ahead of the per-feature kernel (which then only fetches the pose chain and the triple)
            hipLaunchKernelGGL(geom4_kernel, dim3((d.Fu + 3) / 4, 1, B), dim3(64), 0, h->stream, d, n, h->x[h->cur], h->t.n_feat, h->t.types, h->t.len, h->t.meas,
                               h->gpose, h->pfinv, h->gvalid, h->slab_bytes, h->bin, (const CamCal*)h->cal);
        launch_feat_build(h, n, rank, world);
    }
    // unsharded: the reduction finishes into [A|b]; sharded: the block is the payload
    launch_gram(h, forms_at(h, n, false, true, world == 1 && combine), n);
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}

// The code object lists its template kernels in the order the host code first names them.  EVERY template kernel of solve9.hip is named here, in
// the order the code object has them: which function below launches which of them then has no bearing on the device code, and
// tools/device_text_md5.sh can tell a host-side change from one that touched a kernel.  (Nothing reads the table.)
[[maybe_unused]] static const void* const kSolve9Order[] = {
    (const void*)solve9_kernel<1, 4>, (const void*)solve9_kernel<2, 3, true>, (const void*)solve9_kernel<2, 3>, (const void*)solve9_chol_kernel<2, 4>,
    (const void*)solve9_chol_kernel<3, 4>, (const void*)solve9_prod_kernel<0>, (const void*)solve9_prod_kernel<1>, (const void*)solve9_sweep_kernel<2, 4>,
    (const void*)solve9_sweep_kernel<3, 4>, (const void*)solve9_prod_kernel<2>, (const void*)solve9_prod_kernel<3>};
// the two single-workgroup factorisations of the split solve, by tiles per side of the padded clone block (NT = 8 | 12)
static void launch_s9_chol(rvio_hip* h, int NT, int n, double* Pc, hipStream_t st) {
    if (NT == 8) hipLaunchKernelGGL((solve9_chol_kernel<2, 4>), dim3(1), dim3(1024), 0, st, h->dc, n, Pc, h->S9scr);
    else hipLaunchKernelGGL((solve9_chol_kernel<3, 4>), dim3(1), dim3(1024), 0, st, h->dc, n, Pc, h->S9scr);
}
static void launch_s9_sweep(rvio_hip* h, int NT, const double* Ab) {
    if (NT == 8) hipLaunchKernelGGL((solve9_sweep_kernel<2, 4>), dim3(1), dim3(1024), 0, h->stream, h->dc, Ab, h->S9scr);
    else hipLaunchKernelGGL((solve9_sweep_kernel<3, 4>), dim3(1), dim3(1024), 0, h->stream, h->dc, Ab, h->S9scr);
}

static void launch_solve(rvio_hip* h, const UpdateForms& f, int n, const double* Ab) {
    const DevCfg& d = h->dc;
    double *xin = h->x[h->cur], *xout = h->x[h->cur ^ 1], *Pc = h->P[h->cur];
    const dim3 gb(1, 1, h->batch);
    const size_t bs = h->slab_bytes;
    const bool roles = f.dx == LPD_ROLES;   // dx = Pc y and the state injection are left to role workgroups of the Joseph launch behind this one
    switch (f.solve) {
    case LPS_NONE: break;
    // one instance: blocked SPD factorisations on the matrix cores (solve9.hip)
    case LPS_SMALL: hipLaunchKernelGGL(solve9_small_kernel, dim3(1), dim3(1024), f.solve_lds.bytes, h->stream, d, h->meta, n, Ab, xin, Pc, h->S9scr, h->W, xout, roles ? h->S9scr + S9_YP_OFF(4) : (double*)nullptr); break;
    case LPS_S9_1_4: hipLaunchKernelGGL((solve9_kernel<1, 4>), gb, dim3(1024), 0, h->stream, d, h->meta, n, Ab, xin, Pc, h->S9scr, h->W, xout, bs, (size_t)0); break;
    case LPS_S9_2_3_PRE: hipLaunchKernelGGL((solve9_kernel<2, 3, true>), gb, dim3(576), 0, h->stream, d, h->meta, n, Ab, xin, Pc, h->S9scr, h->W, xout, bs, (size_t)0, roles ? 1 : 0); break;
    case LPS_S9_2_3: hipLaunchKernelGGL((solve9_kernel<2, 3>), gb, dim3(576), 0, h->stream, d, h->meta, n, Ab, xin, Pc, h->S9scr, h->W, xout, bs, (size_t)0, roles ? 1 : 0); break;
    case LPS_SPLIT: {   // the four product phases as launches that fill the chip, the two factorisations as one workgroup each
        const int NT = f.split_nt, nwg = (NT * NT + 3) / 4;
        if (f.own_chol) launch_s9_chol(h, NT, n, Pc, h->stream);
        hipLaunchKernelGGL(solve9_prod_kernel<0>, dim3(nwg), dim3(256), 0, h->stream, d, n, Ab, h->S9scr, h->W, NT);
        hipLaunchKernelGGL(solve9_prod_kernel<1>, dim3(nwg), dim3(256), 0, h->stream, d, n, Ab, h->S9scr, h->W, NT);
        launch_s9_sweep(h, NT, Ab);
        hipLaunchKernelGGL(solve9_prod_kernel<2>, dim3(nwg), dim3(256), 0, h->stream, d, n, Ab, h->S9scr, h->W, NT);
        hipLaunchKernelGGL(solve9_prod_kernel<3>, dim3(nwg), dim3(256), 0, h->stream, d, n, Ab, h->S9scr, h->W, NT);
        if (f.dx == LPD_KERNEL) hipLaunchKernelGGL(solve9_dx_kernel, dim3(1), dim3(1024), 0, h->stream, d, h->meta, n, Ab, xin, Pc, h->S9scr, h->W, xout, NT);
        break;
    }
    // batch handles.  Beyond solve6's windows (6n > 126) the register-tableau solve: T = s2 I + A Pcc is formed by the kernel itself
    case LPS_SOLVE7: hipLaunchKernelGGL((solve7_kernel<3, 16, 12>), gb, dim3(768), 0, h->stream, d, h->meta, n, Ab, xin, Pc, h->Tbuf, h->W, xout, bs); break;
    case LPS_SOLVE6_1: hipLaunchKernelGGL((solve6_kernel<1, 8, 8>), gb, dim3(512), f.solve_lds.bytes, h->stream, d, h->meta, n, h->Tbuf, Ab, xin, Pc, h->W, xout, bs); break;
    case LPS_SOLVE6_2: hipLaunchKernelGGL((solve6_kernel<2, 12, 8>), gb, dim3(512), f.solve_lds.bytes, h->stream, d, h->meta, n, h->Tbuf, Ab, xin, Pc, h->W, xout, bs); break;
    case LPS_SOLVE6_3: hipLaunchKernelGGL((solve6_kernel<2, 16, 8>), gb, dim3(512), f.solve_lds.bytes, h->stream, d, h->meta, n, h->Tbuf, Ab, xin, Pc, h->W, xout, bs); break;
    }
}

// U = Pc W, G = U A  (K H = [0 | G]);  Joseph form (Updater.cc:615-619): P1 = (I-KH) P,  P+ = sym(P1 - P1c G^T + s2 G U^T)
// ug, fin: the stages to launch (both: a whole update; the one-launch forms exist for a whole update only).  roles: the solve of these forms ran ahead
// and left dx = Pc y and the state injection to f.role_wgs more workgroups of the first launch.
static void launch_ug_final(rvio_hip* h, const UpdateForms& f, int n, const double* Ab, double* Pn, bool ug, bool fin, bool roles) {
    const DevCfg& d = h->dc;
    const int B = h->batch;
    const size_t bs = h->slab_bytes;
    double* Pc = h->P[h->cur];
    const int role_wgs = roles ? f.role_wgs : 0;
    const double *nod = nullptr, *yp = role_wgs ? (const double*)h->S9scr : nod;
    switch (f.joseph) {
    case LPJ_BATCH: hipLaunchKernelGGL(joseph_batch_kernel, dim3(1, 1, B), dim3(JB_THREADS), f.ug_lds.bytes, h->stream, d, n, Pc, h->W, Ab, Pn, bs); break;
    case LPJ_LDS: hipLaunchKernelGGL(joseph_lds_kernel, dim3(f.grid[0] + role_wgs), dim3(LP_JL_THREADS), f.ug_lds.bytes, h->stream, d, n, Pc, h->W, Ab, Pn, h->meta, (const double*)h->x[h->cur], h->x[h->cur ^ 1], yp, f.grid[0], h->plan.solve9_nt); break;
    case LPJ_LDS_PAIR:
        if (ug) hipLaunchKernelGGL(ug_lds_kernel, dim3(f.grid[0]), dim3(256), f.ug_lds.bytes, h->stream, d, n, Pc, h->W, Ab, h->U, h->G, h->Pt1);
        if (fin) hipLaunchKernelGGL(final_lds_kernel, dim3(f.grid[1]), dim3(256), f.fin_lds.bytes, h->stream, d, n, h->Pt1, h->G, h->U, Pn);
        break;
    case LPJ_TILE:
        if (ug) {
            hipLaunchKernelGGL(ug_tile_kernel<0>, dim3(f.grid[0] + role_wgs), dim3(256), 0, h->stream, d, n, Pc, h->W, Ab, h->U, h->G, h->Pt1,
                               h->meta, (const double*)h->x[h->cur], h->x[h->cur ^ 1], yp, h->plan.solve9_nt);
            hipLaunchKernelGGL(ug_tile_kernel<1>, dim3(f.grid[1]), dim3(256), 0, h->stream, d, n, Pc, h->W, Ab, h->U, h->G, h->Pt1, h->meta, nod, (double*)nullptr, nod, 0);
            hipLaunchKernelGGL(ug_tile_kernel<2>, dim3(f.grid[2]), dim3(256), 0, h->stream, d, n, Pc, h->W, Ab, h->U, h->G, h->Pt1, h->meta, nod, (double*)nullptr, nod, 0);
        }
        if (fin) hipLaunchKernelGGL(final_tile_kernel, dim3(f.grid[3]), dim3(256), 0, h->stream, d, n, h->Pt1, h->G, h->U, Pn);
        break;
    case LPJ_STRIPS:
        if (ug) hipLaunchKernelGGL(ug_kernel, dim3(f.grid[0], 1, B), dim3(256), f.ug_lds.bytes, h->stream, d, n, Pc, h->W, Ab, h->U, h->G, h->Pt1, bs);
        if (fin) hipLaunchKernelGGL(final_kernel, dim3(f.grid[1], 1, B), dim3(256), 0, h->stream, d, n, h->Pt1, h->G, h->U, Pn, bs);
        break;
    }
}

// Updater::update's landmark cloud behind the update just enqueued (h->cur already toggled): one workgroup per instance, a lane per feature slot
static void launch_landmarks(rvio_hip* h, int n, const LmOut& out) {
    const int T = std::min(LM_MAX_T, 64 * ((h->dc.Fu + 63) / 64));
    hipLaunchKernelGGL(landmark_kernel, dim3(1, 1, h->batch), dim3(T), 0, h->stream, h->dc, n, (const double*)h->x[h->cur ^ 1], (const double*)h->x[h->cur],
                       (const int*)h->t.n_feat, (const unsigned char*)h->t.types, (const int*)h->t.len, (const int*)h->acc, (const double*)h->pfinv,
                       h->slab_bytes, h->bin, out, (const CamCal*)h->cal);
}
// grid / workgroup of a front-end launch as front_forms() (launch_plan.h) fixed them
static dim3 lp_grid(const LpLaunch& l) { return dim3((unsigned)l.gx, (unsigned)l.gy, (unsigned)l.gz); }
static dim3 lp_block(const LpLaunch& l) { return dim3((unsigned)l.threads); }
static_assert(sizeof(rvio_landmark_cov) == 8 * LP_LMC_WORDS, "include/rvio_hip.h: rvio_landmark_cov has no padding");
// landmark_cov_kernel behind landmark_kernel (h->cur already toggled): the cloud `cloud` as that launch left it, the state AND covariance the
// update read (x[cur ^ 1], P[cur ^ 1]: every update form writes the other buffers; augcomp_kernel2 rewrites these next), Fu records per instance
static void launch_landmark_cov(rvio_hip* h, int n, const LmOut& cloud, rvio_landmark_cov* rec) {
    const LpLaunch l = landmark_cov_launch(h->batch, h->dc.Fu);
    hipLaunchKernelGGL(landmark_cov_kernel, lp_grid(l), lp_block(l), l.lds, h->stream, h->dc, n, h->dc.dmax, (const double*)h->x[h->cur ^ 1], (const double*)h->P[h->cur ^ 1],
                       (const unsigned char*)h->t.types, (const int*)h->t.len, (const double*)h->pfinv, h->slab_bytes, h->bin, cloud, (const CamCal*)h->cal,
                       LmcOut{(unsigned long long*)rec, (size_t)h->dc.Fu});
}
// cornerSubPix on the detector's raw corners, in the form f names (frame: the instrumented build's stamp)
static void launch_subpix(rvio_hip* h, const FrontForms& f, const DetDev& q, const uint8_t* img, int stride, size_t src_bs, int frame, hipStream_t st) {
    const size_t bs = h->slab_bytes;
    const LpLaunch& l = f.subpix_l;
    switch (f.subpix) {
    case LPSP_NONE: break;
    case LPSP_WIDE_WIN: hipLaunchKernelGGL(subpix_wide_kernel, lp_grid(l), lp_block(l), l.lds, st, img, stride, q, src_bs, bs); break;
    case LPSP_GENERIC: hipLaunchKernelGGL(subpix_generic_kernel, lp_grid(l), lp_block(l), 0, st, img, stride, q, src_bs, bs); break;
    case LPSP_X16: hipLaunchKernelGGL(subpix_kernel16, lp_grid(l), lp_block(l), 0, st, img, stride, q, src_bs, bs); break;
    case LPSP_STOCK: hipLaunchKernelGGL(subpix_kernel, lp_grid(l), lp_block(l), 0, st, img, stride, q, src_bs, bs, frame); break;
    }
}
// the cloud buffers of every instance in one allocation (count | feat[Fu] | p_r[Fu][3] | p_w[Fu][3], 256-byte aligned parts)
static int lm_alloc(rvio_hip* h, LmOut* out) {
    const size_t Fu = (size_t)h->dc.Fu;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_feat = 256, o_pr = o_feat + up(sizeof(int) * Fu), o_pw = o_pr + up(sizeof(double) * 3 * Fu), bs = o_pw + up(sizeof(double) * 3 * Fu);
    char* p = nullptr;
    RCCHK(own_dev(h, &p, bs * h->batch, true));
    *out = LmOut{(int*)p, (int*)(p + o_feat), (double*)(p + o_pr), (double*)(p + o_pw), bs};
    return RVIO_OK;
}

// combined: d_blocks is the handle's own block, already turned into [A|b] by gram_reduce_kernel (unsharded update)
static int update_global_dev(rvio_hip* h, const double* d_blocks, int world, bool combined) {
    const DevCfg& d = h->dc;
    const int n = h->n_clones_host, c6 = 6 * n;
    const long ldh = d.ldh;
    double* Pc = h->P[h->cur];
    double* Pn = h->P[h->cur ^ 1];
    const double* Ab = d_blocks;
    const size_t bs = h->slab_bytes;
    const int B = h->batch;
    if (B > 1 && !combined) { h->err = "a batch handle runs the unsharded updater only"; return RVIO_ERR_UNSUPPORTED; }
    if (!combined) {   // gathered shards [S2 | S1]: sum both parts in rank order, then the rank truncation -> Ab = [A|b]
        const int eg = std::max(1, std::min(64, (int)((c6 * ldh + 255) / 256)));
        hipLaunchKernelGGL(block_sum_kernel, dim3(eg), dim3(256), h->plan.trunc_lds, h->stream, d, n, d_blocks, world, (size_t)shard_payload_doubles(c6, d.max_len), h->Ab, h->gram_cnt,
                           (const int*)h->nrows, (const unsigned char*)h->t.types, (const int*)h->t.len, lit_args(h, h->plan.trunc_lds));
        Ab = h->Ab;
    }
    // the forms of this update, decided once: the solve and the Joseph stage see the same value (who runs dx = Pc y is settled between them here)
    const UpdateForms f = forms_at(h, n, take_chol(h), true, combined);
    if (f.tprod == LPT_GEMM_LDS)
        hipLaunchKernelGGL(gemm_T_lds_kernel, dim3(1, 1, B), dim3(256), f.tprod_lds.bytes, h->stream, d, n, Ab, Pc, h->Tbuf, bs);
    else if (f.tprod == LPT_GEMM)
        hipLaunchKernelGGL(gemm_T_kernel, dim3(f.tprod_grid, f.tprod_grid, B), dim3(256), 0, h->stream, d, n, Ab, Pc, h->Tbuf, bs);
    h->last_Ab = Ab;
    launch_solve(h, f, n, Ab);
    launch_ug_final(h, f, n, Ab, Pn, true, true, f.dx == LPD_ROLES);
    HIPCHK(h, hipGetLastError());
    h->cur ^= 1;
    if (h->lm_on) {   // the cloud: x[cur] is xk1k1 now, x[cur ^ 1] still xk1k (every update form writes the other buffer; augcomp_kernel2 rewrites it next)
        launch_landmarks(h, n, h->lm);
        if (h->lmc_on) launch_landmark_cov(h, n, h->lm, h->lmc);
        HIPCHK(h, hipGetLastError());
        h->lm_frame = h->img_count;
        if (h->lmc_on) h->lmc_frame = h->lm_frame;
    }
    return RVIO_OK;
}

int rvio_hip_update_tracked(rvio_hip* h) {
    if (!h) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = update_local_dev(h, 0, 1, true);
    if (rc != RVIO_OK) return rc;
    return update_global_dev(h, h->block, 1, true);
}
int rvio_hip_update(rvio_hip* h, const rvio_tracks* tracks) {
    if (!h) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = upload_tracks(h, tracks);
    if (rc != RVIO_OK) return rc;
    return rvio_hip_update_tracked(h);
}
int rvio_hip_update_local(rvio_hip* h, const rvio_tracks* tracks, int rank, int world, double** d_block, int* n_doubles) {
    if (!h || world < 1 || rank < 0 || rank >= world) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    if (tracks) { int rc = upload_tracks(h, tracks); if (rc != RVIO_OK) return rc; }
    int rc = update_local_dev(h, rank, world, false);
    if (d_block) *d_block = h->block;
    if (n_doubles) *n_doubles = shard_payload_doubles(6 * h->n_clones_host, h->dc.max_len);
    return rc;
}
int rvio_hip_update_global(rvio_hip* h, const double* d_blocks, int world) {
    if (!h || !d_blocks || world < 1) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    return update_global_dev(h, d_blocks, world, false);
}

int rvio_hip_get_update_diag(rvio_hip* h, int32_t* n_feat, int32_t* accepted, double* gamma, int32_t* ndof, double* pfinv) {
    if (!h) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    SYNC_FRONT(h);   // image / side / tracker streams first
    int nf = 0;
    HIPCHK(h, hipMemcpyAsync(&nf, h->t.n_feat, sizeof nf, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n_feat) *n_feat = nf;
    if (nf > 0) {
        if (accepted) HIPCHK(h, hipMemcpyAsync(accepted, h->acc, sizeof(int) * nf, hipMemcpyDeviceToHost, h->stream));
        if (gamma) HIPCHK(h, hipMemcpyAsync(gamma, h->gamma, sizeof(double) * nf, hipMemcpyDeviceToHost, h->stream));
        if (ndof) HIPCHK(h, hipMemcpyAsync(ndof, h->ndof, sizeof(int) * nf, hipMemcpyDeviceToHost, h->stream));
        if (pfinv) HIPCHK(h, hipMemcpyAsync(pfinv, h->pfinv, sizeof(double) * 3 * nf, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}

// ------------------------------------------------------------------ landmark cloud (Updater.cc:78-87,430-448,458)
int rvio_hip_set_landmarks(rvio_hip* h, int enable) {
    if (!h) return RVIO_ERR_INVALID;
    if (enable && !h->lm.count) {   // first enable: the buffers are allocated with nothing in flight
        { const int rc = drain_all(h); if (rc != RVIO_OK) return rc; }
        { const int rc = lm_alloc(h, &h->lm); if (rc != RVIO_OK) return rc; }
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->lm_on = enable != 0;
    if (!h->lm_on) h->lmc_on = false;   // (the covariance follows the cloud: without one there is nothing it could describe)
    return RVIO_OK;
}
int rvio_hip_get_landmarks_at(rvio_hip* h, int instance, int32_t* n, int32_t* frame, int32_t* feat, double* p_r, double* p_world) {
    if (!h || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    if (!h->lm.count) { h->err = "the landmark cloud was never enabled (rvio_hip_set_landmarks)"; return RVIO_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    SYNC_FRONT(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t o = (size_t)instance * h->lm.bs;
    int cnt = 0;
    if (h->lm_frame >= 0) {
        HIPCHK(h, hipMemcpyAsync(&cnt, (char*)h->lm.count + o, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        cnt = std::max(0, std::min(cnt, h->dc.Fu));
    }
    if (n) *n = cnt;
    if (frame) *frame = h->lm_frame;
    if (cnt > 0) {
        if (feat) HIPCHK(h, hipMemcpyAsync(feat, (char*)h->lm.feat + o, sizeof(int) * cnt, hipMemcpyDeviceToHost, h->stream));
        if (p_r) HIPCHK(h, hipMemcpyAsync(p_r, (char*)h->lm.p_r + o, sizeof(double) * 3 * cnt, hipMemcpyDeviceToHost, h->stream));
        if (p_world) HIPCHK(h, hipMemcpyAsync(p_world, (char*)h->lm.p_w + o, sizeof(double) * 3 * cnt, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return RVIO_OK;
}
int rvio_hip_get_landmarks(rvio_hip* h, int32_t* n, int32_t* frame, int32_t* feat, double* p_r, double* p_world) {
    return rvio_hip_get_landmarks_at(h, 0, n, frame, feat, p_r, p_world);
}

// ------------------------------------------------------------------ landmark covariance (landmark_cov.hip)
int rvio_hip_set_landmark_cov(rvio_hip* h, int enable) {
    if (!h) return RVIO_ERR_INVALID;
    if (enable) {
        if (!h->lm_on) RCCHK(rvio_hip_set_landmarks(h, 1));
        if (!h->lmc) {   // first enable: allocated with nothing in flight, cleared (a record past the cloud's count is never handed out)
            { const int rc = drain_all(h); if (rc != RVIO_OK) return rc; }
            RCCHK(own_dev(h, &h->lmc, sizeof(rvio_landmark_cov) * (size_t)h->dc.Fu * h->batch, true));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
    }
    h->lmc_on = enable != 0;
    return RVIO_OK;
}
int rvio_hip_get_landmark_cov_at(rvio_hip* h, int instance, int32_t* n, int32_t* frame, rvio_landmark_cov* rec) {
    if (!h || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    if (!h->lmc) { h->err = "the landmark covariance was never enabled (rvio_hip_set_landmark_cov)"; return RVIO_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    SYNC_FRONT(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int cnt = 0;
    // (a cloud published while the covariance was off has no records: n = 0 under the stamp of the last cloud that has)
    if (h->lmc_frame >= 0 && h->lmc_frame == h->lm_frame) {
        HIPCHK(h, hipMemcpyAsync(&cnt, (char*)h->lm.count + (size_t)instance * h->lm.bs, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        cnt = std::max(0, std::min(cnt, h->dc.Fu));
    }
    if (n) *n = cnt;
    if (frame) *frame = h->lmc_frame;
    if (cnt > 0 && rec) {
        HIPCHK(h, hipMemcpyAsync(rec, h->lmc + (size_t)instance * h->dc.Fu, sizeof(rvio_landmark_cov) * cnt, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return RVIO_OK;
}
int rvio_hip_get_landmark_cov(rvio_hip* h, int32_t* n, int32_t* frame, rvio_landmark_cov* rec) {
    return rvio_hip_get_landmark_cov_at(h, 0, n, frame, rec);
}
int rvio_hip_get_landmark_cov_dev(rvio_hip* h, rvio_landmark_cov* d_out, size_t out_stride, int32_t* d_count) {
    if (!h) return RVIO_ERR_INVALID;
    if (!d_out) { h->err = "rvio_hip_get_landmark_cov_dev: NULL d_out"; return RVIO_ERR_INVALID; }
    if (out_stride < (size_t)h->dc.Fu) { h->err = "rvio_hip_get_landmark_cov_dev: out_stride is below the handle's hand-over slots"; return RVIO_ERR_INVALID; }
    if (!h->lmc) { h->err = "the landmark covariance was never enabled (rvio_hip_set_landmark_cov)"; return RVIO_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t row = sizeof(rvio_landmark_cov) * (size_t)h->dc.Fu;
    HIPCHK(h, hipMemcpy2DAsync(d_out, sizeof(rvio_landmark_cov) * out_stride, h->lmc, row, row, (size_t)h->batch, hipMemcpyDeviceToDevice, h->stream));
    if (d_count) {
        if (h->lmc_frame >= 0 && h->lmc_frame == h->lm_frame) HIPCHK(h, hipMemcpy2DAsync(d_count, sizeof(int32_t), h->lm.count, h->lm.bs, sizeof(int32_t), (size_t)h->batch, hipMemcpyDeviceToDevice, h->stream));
        else HIPCHK(h, hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)h->batch, h->stream));
    }
    return RVIO_OK;
}

// ------------------------------------------------------------------ odometry ring (System.cc:402-434)
// odom_kernel on the composed state of every instance (h->cur already toggled), into `slot` (batch records)
static void launch_odom(rvio_hip* h, rvio_odom* slot, long long seq) {
    hipLaunchKernelGGL(odom_kernel, dim3((h->batch + 3) / 4), dim3(256), 0, h->stream, h->batch, h->dc.dmax, (const double*)h->x[h->cur], (const double*)h->P[h->cur],
                       (const double*)h->d_pose, h->slab_bytes, seq, h->img_count, h->n_clones_host, (unsigned long long*)slot);
}
// The two operations of a DevRing (the odometry ring here, the IMU-rate ring below).  Capacity: 0 switches the launches off and keeps the ring and
// its records; the capacity it has only switches them on; another one (or the first) is allocated with nothing in flight, and a new ring is empty.
extern "C++" {
// a ring may take 1 GiB (also asked ahead of ring_set_capacity where two rings change together: both or neither)
template <typename T>
static bool ring_too_large(rvio_hip* h, const DevRing<T>& r, int capacity) {
    const size_t bytes = (size_t)capacity * h->batch * sizeof(T);
    if (bytes <= ((size_t)1 << 30)) return false;
    h->err = std::string(r.noun) + " ring of " + std::to_string(capacity) + " x " + std::to_string(h->batch) + " records = " + std::to_string(bytes) + " bytes exceeds 1 GiB";
    return true;
}
template <typename T>
static int ring_set_capacity(rvio_hip* h, DevRing<T>& r, int capacity, int limit) {
    if (capacity < 0 || capacity > limit) return RVIO_ERR_INVALID;
    if (capacity == 0) { r.on = false; return RVIO_OK; }
    if (capacity != r.cap) {
        if (ring_too_large(h, r, capacity)) return RVIO_ERR_UNSUPPORTED;
        const size_t bytes = (size_t)capacity * h->batch * sizeof(T);
        { const int rc = drain_all(h); if (rc != RVIO_OK) return rc; }
        RCCHK(own_replace(h, &r.ring, bytes));
        r.cap = capacity; r.seq = 0;
        HIPCHK(h, hipMemsetAsync(r.ring, 0, bytes, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    r.on = true;
    return RVIO_OK;
}
template <typename T>
static bool ring_exists(rvio_hip* h, const DevRing<T>& r) {
    if (!r.ring) h->err = std::string("the ") + r.noun + " ring was never enabled (" + r.setter + ")";
    return r.ring != nullptr;
}
// Up to max_n records of one instance from first_seq on, oldest first (ring_span.h: at most two spans; instance i's records lie batch records
// apart).  The filter stream only, like rvio_hip_get_pose: every record is written on it, or on a stream it has joined since (the overlapped
// propagate of rvio_hip_frame_tracks_dev)
template <typename T>
static int ring_read(rvio_hip* h, const DevRing<T>& r, int instance, int64_t first_seq, int max_n, T* out, int32_t* n) {
    if (instance < 0 || instance >= h->batch || max_n < 0 || (!out && max_n > 0)) return RVIO_ERR_INVALID;
    if (!ring_exists(h, r)) return RVIO_ERR_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    const RingSpan s = ring_span(r.seq, r.cap, first_seq, max_n);
    if (n) *n = (int32_t)s.count;
    if (s.count == 0) return RVIO_OK;
    const size_t pitch = sizeof(T) * h->batch;
    HIPCHK(h, hipMemcpy2DAsync(out, sizeof(T), r.ring + (size_t)s.slot0 * h->batch + instance, pitch, sizeof(T), (size_t)s.n0, hipMemcpyDeviceToHost, h->stream));
    if (s.count > s.n0)
        HIPCHK(h, hipMemcpy2DAsync(out + s.n0, sizeof(T), r.ring + instance, pitch, sizeof(T), (size_t)(s.count - s.n0), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}
}  // extern "C++"
int rvio_hip_set_odometry(rvio_hip* h, int capacity) { return h ? ring_set_capacity(h, h->odom, capacity, 65536) : RVIO_ERR_INVALID; }
int rvio_hip_get_odometry(rvio_hip* h, int instance, int64_t first_seq, int max_n, rvio_odom* out, int32_t* n) {
    return h ? ring_read(h, h->odom, instance, first_seq, max_n, out, n) : RVIO_ERR_INVALID;
}
int rvio_hip_get_odometry_all(rvio_hip* h, rvio_odom* out, int64_t* seq) {
    if (!h || !out) return RVIO_ERR_INVALID;
    if (!ring_exists(h, h->odom)) return RVIO_ERR_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    if (seq) *seq = h->odom.seq;
    if (h->odom.seq == 0) return RVIO_OK;
    HIPCHK(h, hipMemcpyAsync(out, h->odom.slot(h->odom.seq, h->batch), sizeof(rvio_odom) * h->batch, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}

// ------------------------------------------------------------------ fixed-lag smoothed trajectory (window_pose.hip)
static_assert(sizeof(rvio_window_pose) == 8 * LP_WINP_WORDS, "include/rvio_hip.h: rvio_window_pose has no padding");
static_assert(RVIO_MAX_LEN - 1 <= LP_FIXP_NMAX, "launch_plan.h: the chain window_pose_kernel holds reaches every window a handle accepts");
// window_pose_kernel on `instances` instances from x / P on (instance z lies slab_bytes behind), ages age_first .. age_first + n_ages - 1, record
// (z, age) into out[z * out_stride + age - age_first]; the filter stream, which owns x and P
static void launch_window_pose(rvio_hip* h, int instances, const double* x, const double* P, int age_first, int n_ages, long long seq, rvio_window_pose* out,
                               size_t out_stride) {
    const LpLaunch l = window_pose_launch(instances, n_ages);
    hipLaunchKernelGGL(window_pose_kernel, lp_grid(l), lp_block(l), l.lds, h->stream, h->n_clones_host, h->dc.dmax, x, P, h->slab_bytes, age_first, h->composed_count,
                       seq, (unsigned long long*)out, out_stride);
}
static int window_check(rvio_hip* h, const char* entry) {
    if (!h->has_state) { h->err = std::string(entry) + " before the first rvio_hip_set_state / rvio_hip_initialize"; return RVIO_ERR_STATE; }
    return RVIO_OK;
}
int rvio_hip_get_window(rvio_hip* h, int instance, int max_n, rvio_window_pose* out, int32_t* n) {
    if (!h) return RVIO_ERR_INVALID;
    if (!out || !n) { h->err = "rvio_hip_get_window: NULL out or n"; return RVIO_ERR_INVALID; }
    if (instance < 0 || instance >= h->batch) { h->err = "rvio_hip_get_window: instance out of range"; return RVIO_ERR_INVALID; }
    if (max_n < 1) { h->err = "rvio_hip_get_window: max_n < 1"; return RVIO_ERR_INVALID; }
    RCCHK(window_check(h, "rvio_hip_get_window"));
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->win_buf) RCCHK(own_dev(h, &h->win_buf, sizeof(rvio_window_pose) * (size_t)(h->dc.nmax + 1)));
    const int cnt = std::min(h->n_clones_host + 1, max_n);
    const size_t off = (size_t)instance * h->slab_bytes;
    launch_window_pose(h, 1, (const double*)((const char*)h->x[h->cur] + off), (const double*)((const char*)h->P[h->cur] + off), 0, cnt, 0, h->win_buf, (size_t)cnt);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->win_buf, sizeof(rvio_window_pose) * (size_t)cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n = cnt;
    return RVIO_OK;
}
int rvio_hip_get_window_dev(rvio_hip* h, int age_first, int n_ages, rvio_window_pose* d_out, size_t out_stride) {
    if (!h) return RVIO_ERR_INVALID;
    if (!d_out) { h->err = "rvio_hip_get_window_dev: NULL d_out"; return RVIO_ERR_INVALID; }
    if (age_first < 0 || n_ages < 1 || n_ages > 65535) { h->err = "rvio_hip_get_window_dev: age_first < 0 or n_ages outside 1 .. 65535"; return RVIO_ERR_INVALID; }
    if (out_stride < (size_t)n_ages) { h->err = "rvio_hip_get_window_dev: out_stride is below n_ages"; return RVIO_ERR_INVALID; }
    RCCHK(window_check(h, "rvio_hip_get_window_dev"));
    HIPCHK(h, hipSetDevice(h->device));
    launch_window_pose(h, h->batch, h->x[h->cur], h->P[h->cur], age_first, n_ages, 0, d_out, out_stride);
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}
// the ring: rvio_hip_set_odometry's clauses; another lag empties a ring that stays (nothing in flight writes it: drained first)
int rvio_hip_set_smoothed_odometry(rvio_hip* h, int capacity, int lag) {
    if (!h) return RVIO_ERR_INVALID;
    if (lag < 0 || lag > h->cfg.max_track_len - 1) { h->err = "rvio_hip_set_smoothed_odometry: lag outside 0 .. max_track_len - 1"; return RVIO_ERR_INVALID; }
    if (capacity < 0 || capacity > 65536) { h->err = "rvio_hip_set_smoothed_odometry: capacity outside 0 .. 65536"; return RVIO_ERR_INVALID; }
    const bool kept = capacity > 0 && capacity == h->smo.cap;
    RCCHK(ring_set_capacity(h, h->smo, capacity, 65536));
    if (capacity == 0) return RVIO_OK;
    if (kept && lag != h->smo_lag) {
        { const int rc = drain_all(h); if (rc != RVIO_OK) return rc; }
        HIPCHK(h, hipMemsetAsync(h->smo.ring, 0, sizeof(rvio_window_pose) * (size_t)h->smo.cap * h->batch, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->smo.seq = 0;
    }
    h->smo_lag = lag;
    return RVIO_OK;
}
int rvio_hip_get_smoothed_odometry(rvio_hip* h, int instance, int64_t first_seq, int max_n, rvio_window_pose* out, int32_t* n) {
    return h ? ring_read(h, h->smo, instance, first_seq, max_n, out, n) : RVIO_ERR_INVALID;
}
int rvio_hip_get_smoothed_odometry_all(rvio_hip* h, rvio_window_pose* out, int64_t* seq) {
    if (!h || !out) return RVIO_ERR_INVALID;
    if (!ring_exists(h, h->smo)) return RVIO_ERR_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    if (seq) *seq = h->smo.seq;
    if (h->smo.seq == 0) return RVIO_OK;
    HIPCHK(h, hipMemcpyAsync(out, h->smo.slot(h->smo.seq, h->batch), sizeof(rvio_window_pose) * h->batch, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}

// ------------------------------------------------------------------ pose-graph export: window edges and joint covariance (window_edge.hip)
static_assert(sizeof(rvio_window_edge) == 8 * LP_WEDGE_WORDS, "include/rvio_hip.h: rvio_window_edge has no padding");
static_assert(LP_WEDGE_MAX_PAIRS == RVIO_MAX_LEN * (RVIO_MAX_LEN + 1) / 2, "launch_plan.h: every pair of the longest window");
// window_edge_kernel on `instances` instances from x / P on, the pairs of the device lists (NULL: the one pair (a0, b0)), record (z, pair) into
// out[z * out_stride + pair]; the filter stream, which owns x and P
static void launch_window_edge(rvio_hip* h, int instances, const double* x, const double* P, int n_pairs, const int* d_new, const int* d_old, int a0, int b0,
                               long long seq, rvio_window_edge* out, size_t out_stride) {
    const LpLaunch l = window_edge_launch(instances, n_pairs);
    hipLaunchKernelGGL(window_edge_kernel, lp_grid(l), lp_block(l), l.lds, h->stream, h->n_clones_host, h->dc.dmax, x, P, h->slab_bytes, d_new, d_old, a0, b0,
                       h->composed_count, seq, (unsigned long long*)out, out_stride);
}
int rvio_hip_get_window_edges(rvio_hip* h, int instance, int n_pairs, const int32_t* age_new, const int32_t* age_old, rvio_window_edge* out) {
    if (!h) return RVIO_ERR_INVALID;
    if (!age_new || !age_old || !out) { h->err = "rvio_hip_get_window_edges: NULL age_new, age_old or out"; return RVIO_ERR_INVALID; }
    if (instance < 0 || instance >= h->batch) { h->err = "rvio_hip_get_window_edges: instance out of range"; return RVIO_ERR_INVALID; }
    if (n_pairs < 1 || n_pairs > LP_WEDGE_MAX_PAIRS) { h->err = "rvio_hip_get_window_edges: n_pairs outside 1 .. 528"; return RVIO_ERR_INVALID; }
    RCCHK(window_check(h, "rvio_hip_get_window_edges"));
    for (int i = 0; i < n_pairs; ++i)
        if (!(age_new[i] >= 0 && age_new[i] < age_old[i] && age_old[i] <= h->n_clones_host)) {
            h->err = "rvio_hip_get_window_edges: pair " + std::to_string(i) + " (" + std::to_string(age_new[i]) + ", " + std::to_string(age_old[i]) +
                     ") is not 0 <= age_new < age_old <= n_clones = " + std::to_string(h->n_clones_host);
            return RVIO_ERR_INVALID;
        }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t rec_bytes = sizeof(rvio_window_edge) * (size_t)LP_WEDGE_MAX_PAIRS, list_bytes = sizeof(int32_t) * (size_t)LP_WEDGE_MAX_PAIRS;
    if (!h->wedge_buf) RCCHK(own_dev(h, &h->wedge_buf, rec_bytes + 2 * list_bytes));
    rvio_window_edge* d_rec = (rvio_window_edge*)h->wedge_buf;
    int* d_new = (int*)(h->wedge_buf + rec_bytes);
    int* d_old = (int*)(h->wedge_buf + rec_bytes + list_bytes);
    HIPCHK(h, hipMemcpyAsync(d_new, age_new, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_old, age_old, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice, h->stream));
    const size_t off = (size_t)instance * h->slab_bytes;
    launch_window_edge(h, 1, (const double*)((const char*)h->x[h->cur] + off), (const double*)((const char*)h->P[h->cur] + off), n_pairs, d_new, d_old, 0, 0, 0,
                       d_rec, (size_t)n_pairs);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, d_rec, sizeof(rvio_window_edge) * (size_t)n_pairs, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}
int rvio_hip_get_window_edges_dev(rvio_hip* h, int n_pairs, const int32_t* d_age_new, const int32_t* d_age_old, rvio_window_edge* d_out, size_t out_stride) {
    if (!h) return RVIO_ERR_INVALID;
    if (!d_age_new || !d_age_old || !d_out) { h->err = "rvio_hip_get_window_edges_dev: NULL d_age_new, d_age_old or d_out"; return RVIO_ERR_INVALID; }
    if (n_pairs < 1 || n_pairs > 65535) { h->err = "rvio_hip_get_window_edges_dev: n_pairs outside 1 .. 65535"; return RVIO_ERR_INVALID; }
    if (out_stride < (size_t)n_pairs) { h->err = "rvio_hip_get_window_edges_dev: out_stride is below n_pairs"; return RVIO_ERR_INVALID; }
    RCCHK(window_check(h, "rvio_hip_get_window_edges_dev"));
    HIPCHK(h, hipSetDevice(h->device));
    launch_window_edge(h, h->batch, h->x[h->cur], h->P[h->cur], n_pairs, d_age_new, d_age_old, 0, 0, 0, d_out, out_stride);
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}
// the ring: rvio_hip_set_smoothed_odometry's clauses; another pair empties a ring that stays
int rvio_hip_set_edge_odometry(rvio_hip* h, int capacity, int age_new, int age_old) {
    if (!h) return RVIO_ERR_INVALID;
    if (!(age_new >= 0 && age_new < age_old && age_old <= h->cfg.max_track_len - 1)) {
        h->err = "rvio_hip_set_edge_odometry: not 0 <= age_new < age_old <= max_track_len - 1"; return RVIO_ERR_INVALID;
    }
    if (capacity < 0 || capacity > 65536) { h->err = "rvio_hip_set_edge_odometry: capacity outside 0 .. 65536"; return RVIO_ERR_INVALID; }
    const bool kept = capacity > 0 && capacity == h->edg.cap;
    RCCHK(ring_set_capacity(h, h->edg, capacity, 65536));
    if (capacity == 0) return RVIO_OK;
    if (kept && (age_new != h->edg_new || age_old != h->edg_old)) {
        { const int rc = drain_all(h); if (rc != RVIO_OK) return rc; }
        HIPCHK(h, hipMemsetAsync(h->edg.ring, 0, sizeof(rvio_window_edge) * (size_t)h->edg.cap * h->batch, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->edg.seq = 0;
    }
    h->edg_new = age_new; h->edg_old = age_old;
    return RVIO_OK;
}
int rvio_hip_get_edge_odometry(rvio_hip* h, int instance, int64_t first_seq, int max_n, rvio_window_edge* out, int32_t* n) {
    return h ? ring_read(h, h->edg, instance, first_seq, max_n, out, n) : RVIO_ERR_INVALID;
}
int rvio_hip_get_edge_odometry_all(rvio_hip* h, rvio_window_edge* out, int64_t* seq) {
    if (!h || !out) return RVIO_ERR_INVALID;
    if (!ring_exists(h, h->edg)) return RVIO_ERR_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    if (seq) *seq = h->edg.seq;
    if (h->edg.seq == 0) return RVIO_OK;
    HIPCHK(h, hipMemcpyAsync(out, h->edg.slot(h->edg.seq, h->batch), sizeof(rvio_window_edge) * h->batch, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}
// window_joint_kernel on `instances` instances from x / P on, ages 0 .. n_ages - 1: pose (z, a) into poses[z * pose_stride + a], instance z's matrix
// (row-major, leading dimension ldc) cov_stride doubles behind instance 0's
static void launch_window_joint(rvio_hip* h, int instances, const double* x, const double* P, int n_ages, rvio_window_pose* poses, size_t pose_stride, double* cov,
                                size_t cov_stride, int ldc) {
    const LpLaunch l = window_joint_launch(instances, n_ages);
    hipLaunchKernelGGL(window_joint_kernel, lp_grid(l), lp_block(l), l.lds, h->stream, h->n_clones_host, h->dc.dmax, x, P, h->slab_bytes, h->composed_count,
                       (unsigned long long*)poses, pose_stride, cov, cov_stride, ldc);
}
int rvio_hip_get_window_joint(rvio_hip* h, int instance, int max_n, rvio_window_pose* poses, double* cov, size_t ld, int32_t* n) {
    if (!h) return RVIO_ERR_INVALID;
    if (!poses || !cov || !n) { h->err = "rvio_hip_get_window_joint: NULL poses, cov or n"; return RVIO_ERR_INVALID; }
    if (instance < 0 || instance >= h->batch) { h->err = "rvio_hip_get_window_joint: instance out of range"; return RVIO_ERR_INVALID; }
    if (max_n < 1) { h->err = "rvio_hip_get_window_joint: max_n < 1"; return RVIO_ERR_INVALID; }
    if (ld < 6 * (size_t)max_n) { h->err = "rvio_hip_get_window_joint: ld is below 6 max_n"; return RVIO_ERR_INVALID; }
    RCCHK(window_check(h, "rvio_hip_get_window_joint"));
    HIPCHK(h, hipSetDevice(h->device));
    const size_t side = 6 * (size_t)(h->dc.nmax + 1), cov_bytes = sizeof(double) * side * side;
    if (!h->wjoint_buf) RCCHK(own_dev(h, &h->wjoint_buf, cov_bytes + sizeof(rvio_window_pose) * (size_t)(h->dc.nmax + 1)));
    double* d_cov = (double*)h->wjoint_buf;
    rvio_window_pose* d_poses = (rvio_window_pose*)(h->wjoint_buf + cov_bytes);
    const int cnt = std::min(h->n_clones_host + 1, max_n);
    const size_t off = (size_t)instance * h->slab_bytes;
    launch_window_joint(h, 1, (const double*)((const char*)h->x[h->cur] + off), (const double*)((const char*)h->P[h->cur] + off), cnt, d_poses, (size_t)cnt, d_cov,
                        0, 6 * cnt);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(poses, d_poses, sizeof(rvio_window_pose) * (size_t)cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpy2DAsync(cov, sizeof(double) * ld, d_cov, sizeof(double) * 6 * (size_t)cnt, sizeof(double) * 6 * (size_t)cnt, 6 * (size_t)cnt,
                               hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n = cnt;
    return RVIO_OK;
}
int rvio_hip_get_window_joint_dev(rvio_hip* h, int n_ages, rvio_window_pose* d_poses, size_t pose_stride, double* d_cov, size_t cov_stride) {
    if (!h) return RVIO_ERR_INVALID;
    if (!d_poses || !d_cov) { h->err = "rvio_hip_get_window_joint_dev: NULL d_poses or d_cov"; return RVIO_ERR_INVALID; }
    if (n_ages < 1 || n_ages > RVIO_MAX_LEN) { h->err = "rvio_hip_get_window_joint_dev: n_ages outside 1 .. 32"; return RVIO_ERR_INVALID; }
    if (pose_stride < (size_t)n_ages) { h->err = "rvio_hip_get_window_joint_dev: pose_stride is below n_ages"; return RVIO_ERR_INVALID; }
    if (cov_stride < 36 * (size_t)n_ages * n_ages) { h->err = "rvio_hip_get_window_joint_dev: cov_stride is below (6 n_ages)^2"; return RVIO_ERR_INVALID; }
    RCCHK(window_check(h, "rvio_hip_get_window_joint_dev"));
    HIPCHK(h, hipSetDevice(h->device));
    launch_window_joint(h, h->batch, h->x[h->cur], h->P[h->cur], n_ages, d_poses, pose_stride, d_cov, cov_stride, 6 * n_ages);
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}

// ------------------------------------------------------------------ IMU-rate odometry (imu_pose.hip)
static int predict_check(rvio_hip* h) {
    if (!h->has_state) { h->err = "rvio_hip_predict before the first rvio_hip_set_state / rvio_hip_initialize"; return RVIO_ERR_STATE; }
    return RVIO_OK;
}
// The device forms, every instance, asynchronous on the filter stream (behind everything enqueued there, ahead of everything enqueued later):
// the pose records where d_out, the covariance records (imu_cov.hip) where d_cov
static int predict_dev(rvio_hip* h, const rvio_imu* d_imu, int imu_stride, int m, rvio_imu_pose* d_out, int out_stride, rvio_imu_cov* d_cov, int cov_stride) {
    { const int rc = predict_check(h); if (rc != RVIO_OK) return rc; }
    if (m == 0) return RVIO_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t imu_bs = (size_t)imu_stride * sizeof(rvio_imu);
    if (d_out) launch_imu_pose(h, h->stream, h->batch, h->x[h->cur], d_imu, imu_bs, m, d_out, out_stride, 0, 0, h->img_count);
    if (d_cov) launch_imu_cov(h, h->stream, h->batch, h->x[h->cur], h->P[h->cur], d_imu, imu_bs, m, d_cov, cov_stride, 0, 0, h->img_count);
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}
int rvio_hip_predict_dev(rvio_hip* h, const rvio_imu* d_imu, int imu_stride, int m, rvio_imu_pose* d_out, int out_stride) {
    if (!h || m < 0 || (m > 0 && (!d_imu || !d_out)) || imu_stride < 0 || (imu_stride > 0 && imu_stride < m) || out_stride < m) return RVIO_ERR_INVALID;
    return predict_dev(h, d_imu, imu_stride, m, d_out, out_stride, nullptr, 0);
}
// d_out == NULL: covariances only
int rvio_hip_predict_cov_dev(rvio_hip* h, const rvio_imu* d_imu, int imu_stride, int m, rvio_imu_pose* d_out, int out_stride, rvio_imu_cov* d_cov, int cov_stride) {
    if (!h || m < 0 || (m > 0 && (!d_imu || !d_cov)) || imu_stride < 0 || (imu_stride > 0 && imu_stride < m) || (d_out && out_stride < m) || cov_stride < m) return RVIO_ERR_INVALID;
    return predict_dev(h, d_imu, imu_stride, m, d_out, out_stride, d_cov, cov_stride);
}
// The staging of the host forms: `cap` samples, pose records and — from the first call that asks for covariance on — covariance records.  It is
// replaced as a whole (all blocks or none; every earlier call has waited for its copies, so nothing reads the old ones)
static int predict_staging(rvio_hip* h, int m, bool with_cov) {
    rvio_hip::PredStage& g = h->pred;
    with_cov = with_cov || g.cov;
    if (m <= g.cap && (g.cov || !with_cov)) return RVIO_OK;
    rvio_hip::PredStage n;
    n.cap = (m <= g.cap) ? g.cap : std::max(std::max(2 * g.cap, RVIO_HIP_MAX_IMU), (m + 63) & ~63);
    int rc = own_dev(h, &n.imu, sizeof(rvio_imu) * (size_t)n.cap);
    if (rc == RVIO_OK) rc = own_dev(h, &n.out, sizeof(rvio_imu_pose) * (size_t)n.cap);
    if (rc == RVIO_OK && with_cov) rc = own_dev(h, &n.cov, sizeof(rvio_imu_cov) * (size_t)n.cap);
    const rvio_hip::PredStage drop = (rc == RVIO_OK) ? g : n;
    own_release(h, drop.imu); own_release(h, drop.out); own_release(h, drop.cov);
    if (rc == RVIO_OK) g = n;
    return rc;
}
// The host forms, one instance: staged through buffers of their own (the staging of the other host-buffer entry points may still be read by a
// frame in flight), which grow with m; they wait for the filter stream only, like rvio_hip_get_pose.  The pose records where out, the
// covariance records where cov
static int predict_host(rvio_hip* h, int instance, const rvio_imu* imu, int m, rvio_imu_pose* out, rvio_imu_cov* cov) {
    { const int rc = predict_check(h); if (rc != RVIO_OK) return rc; }
    if (m == 0) return RVIO_OK;
    HIPCHK(h, hipSetDevice(h->device));
    RCCHK(predict_staging(h, m, cov != nullptr));
    const auto& g = h->pred;
    const size_t off = (size_t)instance * h->slab_bytes;
    const double *xi = (const double*)((const char*)h->x[h->cur] + off), *Pi = (const double*)((const char*)h->P[h->cur] + off);
    HIPCHK(h, hipMemcpyAsync(g.imu, imu, sizeof(rvio_imu) * (size_t)m, hipMemcpyHostToDevice, h->stream));
    if (out) launch_imu_pose(h, h->stream, 1, xi, g.imu, 0, m, g.out, m, 0, 0, h->img_count);
    if (cov) launch_imu_cov(h, h->stream, 1, xi, Pi, g.imu, 0, m, g.cov, m, 0, 0, h->img_count);
    HIPCHK(h, hipGetLastError());
    if (out) HIPCHK(h, hipMemcpyAsync(out, g.out, sizeof(rvio_imu_pose) * (size_t)m, hipMemcpyDeviceToHost, h->stream));
    if (cov) HIPCHK(h, hipMemcpyAsync(cov, g.cov, sizeof(rvio_imu_cov) * (size_t)m, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}
int rvio_hip_predict(rvio_hip* h, int instance, const rvio_imu* imu, int m, rvio_imu_pose* out) {
    if (!h || instance < 0 || instance >= h->batch || m < 0 || (m > 0 && (!imu || !out))) return RVIO_ERR_INVALID;
    return predict_host(h, instance, imu, m, out, nullptr);
}
// out == NULL: covariances only
int rvio_hip_predict_cov(rvio_hip* h, int instance, const rvio_imu* imu, int m, rvio_imu_pose* out, rvio_imu_cov* cov) {
    if (!h || instance < 0 || instance >= h->batch || m < 0 || (m > 0 && (!imu || !cov))) return RVIO_ERR_INVALID;
    return predict_host(h, instance, imu, m, out, cov);
}
// the ring: rvio_hip_set_odometry's clauses, one record per IMU sample instead of one per frame
// (a covariance ring that exists follows every change of capacity: both rings are reallocated and emptied, or neither)
int rvio_hip_set_imu_odometry(rvio_hip* h, int capacity) {
    if (!h) return RVIO_ERR_INVALID;
    const bool both = h->imuc.ring && capacity > 0 && capacity <= 1048576 && capacity != h->imuo.cap;
    if (both && ring_too_large(h, h->imuc, capacity)) return RVIO_ERR_UNSUPPORTED;
    RCCHK(ring_set_capacity(h, h->imuo, capacity, 1048576));
    if (both) {
        const bool on = h->imuc.on;
        RCCHK(ring_set_capacity(h, h->imuc, capacity, 1048576));
        h->imuc.on = on; h->imuc_first = 1;
    }
    return RVIO_OK;
}
int rvio_hip_get_imu_odometry(rvio_hip* h, int instance, int64_t first_seq, int max_n, rvio_imu_pose* out, int32_t* n) {
    return h ? ring_read(h, h->imuo, instance, first_seq, max_n, out, n) : RVIO_ERR_INVALID;
}
// the covariance ring beside it: the IMU-rate ring's capacity, seq and slots
int rvio_hip_set_imu_odometry_cov(rvio_hip* h, int enable) {
    if (!h || (enable != 0 && enable != 1)) return RVIO_ERR_INVALID;
    if (!enable) { h->imuc.on = false; return RVIO_OK; }
    if (!ring_exists(h, h->imuo)) return RVIO_ERR_STATE;
    if (h->imuc.on) return RVIO_OK;
    if (h->imuc.cap != h->imuo.cap) {
        if (ring_too_large(h, h->imuc, h->imuo.cap)) return RVIO_ERR_UNSUPPORTED;
        RCCHK(ring_set_capacity(h, h->imuc, h->imuo.cap, 1048576));
    }
    h->imuc.on = true;
    h->imuc_first = h->imuo.seq + 1;   // the getter serves what is recorded from here on
    return RVIO_OK;
}
int rvio_hip_get_imu_odometry_cov(rvio_hip* h, int instance, int64_t first_seq, int max_n, rvio_imu_cov* out, int32_t* n) {
    if (!h) return RVIO_ERR_INVALID;
    return ring_read(h, h->imuc, instance, std::max<int64_t>(first_seq, h->imuc_first), max_n, out, n);
}

// ------------------------------------------------------------------ auxiliary measurement update (aux_update.hip)
static_assert(LP_AUX_MAX_ROWS == RVIO_AUX_MAX_ROWS, "launch_plan.h: the row limit of the auxiliary update");
// ---- what the measurement updates share (this section, standstill, fixes, past-frame fixes): one way in — entry guard, host staging, active
// flags — and one way out, the (gamma, applied) pair aux_update_kernel leaves
// the two state errors of a public call, once per call and in front of anything it enqueues; `entry` names it in the message
static int meas_guard(rvio_hip* h, const char* entry) {
    if (!h->has_state) { h->err = std::string(entry) + " before the first rvio_hip_set_state / rvio_hip_initialize"; return RVIO_ERR_STATE; }
    if (h->in_frame) { h->err = std::string(entry) + " between rvio_hip_frame_begin_dev and rvio_hip_frame_end"; return RVIO_ERR_STATE; }
    return RVIO_OK;
}
// The first use allocates the three parts (all or none: a failure half-way leaves the members null, and the next call starts over); a later
// one waits until the previous call's copy has left the pinned block.  `bytes` is fixed per handle and entry point
static int stage_acquire(rvio_hip* h, HostStage& s, size_t bytes) {
    if (s.pin) { HIPCHK(h, hipEventSynchronize(s.ev)); return RVIO_OK; }
    HostStage t;
    int rc = own_pinned(h, &t.pin, bytes);
    if (rc == RVIO_OK) rc = own_dev(h, &t.dev, bytes);
    if (rc == RVIO_OK) rc = own_event(h, &t.ev, hipEventDisableTiming);
    if (rc != RVIO_OK) { own_release(h, t.pin); own_release(h, t.dev); return rc; }
    s = t;
    return RVIO_OK;
}
// The last int32 per instance of every staged block are the active flags of the host forms' `instance`: one instance, or -1 for all of them.
// Fills them, then copies the block on the filter stream, where it is consumed — no wait for the stream itself.  *d_active: what the launch
// gets, the flags' device twin, or with -1 no flags at all
static int stage_send(rvio_hip* h, const HostStage& s, size_t bytes, int instance, const int32_t** d_active) {
    const size_t at = bytes - sizeof(int32_t) * (size_t)h->batch;
    for (int i = 0; i < h->batch; ++i) ((int32_t*)(s.pin + at))[i] = (instance < 0 || i == instance) ? 1 : 0;
    *d_active = instance < 0 ? nullptr : (const int32_t*)(s.dev + at);
    HIPCHK(h, hipMemcpyAsync(s.dev, s.pin, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(s.ev, h->stream));
    return RVIO_OK;
}
// (gamma, applied) of one instance as the last aux launch left them at d_pair, behind `rec_bytes` of a record copied from the same stream;
// waits for the filter stream only, like rvio_hip_get_pose
static int read_pair(rvio_hip* h, const double* d_pair, int instance, double* gamma, long long* applied, void* rec = nullptr, const void* d_rec = nullptr, size_t rec_bytes = 0) {
    HIPCHK(h, hipSetDevice(h->device));
    double dg[2];
    if (rec) HIPCHK(h, hipMemcpyAsync(rec, d_rec, rec_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(dg, d_pair + 2 * (size_t)instance, sizeof dg, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *gamma = dg[0];
    std::memcpy(applied, &dg[1], sizeof *applied);
    return RVIO_OK;
}

// The bare launch, behind its caller's guard.  Strides in doubles (0: shared).  Asynchronous on the filter stream: in place on x[cur] / P[cur],
// no toggle.  d_diag: (gamma, applied) go there instead of aux.diag (the standstill and fix updates keep their own)
static int update_aux_dev(rvio_hip* h, int m, int mode, int gate, const double* d_H, size_t H_stride, const double* d_v, size_t v_stride,
                          const double* d_sigma, size_t sigma_stride, const int32_t* d_active, double* d_diag = nullptr) {
    if (!d_diag) {
        if (!h->aux.diag) RCCHK(own_dev(h, &h->aux.diag, sizeof(double) * 2 * (size_t)h->batch, true));
        d_diag = h->aux.diag;
    }
    RCCHK(chol_drop(h, CHOL_FILTER_WAITS));   // (the update changes the covariance in place)
    const int n = h->n_clones_host;
    const LpLaunch l = aux_update_launch(n, m, h->batch);
    const size_t w = sizeof(double);
    if (l.kernel == LPK_AUX_UPDATE4)
        hipLaunchKernelGGL(aux_update_kernel<4>, lp_grid(l), lp_block(l), l.lds, h->stream, n, h->dc.dmax, m, mode, gate, h->x[h->cur], h->P[h->cur], h->d_pose, h->meta,
                           h->slab_bytes, d_H, H_stride * w, d_v, v_stride * w, d_sigma, sigma_stride * w, (const int*)d_active, d_diag);
    else
        hipLaunchKernelGGL(aux_update_kernel<16>, lp_grid(l), lp_block(l), l.lds, h->stream, n, h->dc.dmax, m, mode, gate, h->x[h->cur], h->P[h->cur], h->d_pose, h->meta,
                           h->slab_bytes, d_H, H_stride * w, d_v, v_stride * w, d_sigma, sigma_stride * w, (const int*)d_active, d_diag);
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}
int rvio_hip_update_aux_dev(rvio_hip* h, int m, int mode, int gate, const double* d_H, size_t H_stride, const double* d_v, size_t v_stride,
                            const double* d_sigma, size_t sigma_stride, const int32_t* d_active) {
    if (!h || !d_H || !d_v || !d_sigma || m < 1 || m > RVIO_AUX_MAX_ROWS || (mode != RVIO_AUX_RESIDUAL && mode != RVIO_AUX_VALUE) || (gate != 0 && gate != 1))
        return RVIO_ERR_INVALID;
    const size_t d = 24 + 6 * (size_t)h->n_clones_host;
    if ((H_stride && H_stride < (size_t)m * d) || (v_stride && v_stride < (size_t)m) || (sigma_stride && sigma_stride < (size_t)m)) return RVIO_ERR_INVALID;
    RCCHK(meas_guard(h, "rvio_hip_update_aux"));
    HIPCHK(h, hipSetDevice(h->device));
    return update_aux_dev(h, m, mode, gate, d_H, H_stride, d_v, v_stride, d_sigma, sigma_stride, d_active);
}
// host buffers: checked here, packed into the pinned block once the copy of the previous call has left it, copied and consumed on the filter
// stream — no wait for the stream itself
int rvio_hip_update_aux(rvio_hip* h, int instance, const rvio_aux_meas* meas) {
    if (!h || !meas || !meas->H || !meas->v || !meas->sigma || instance < -1 || instance >= h->batch) return RVIO_ERR_INVALID;
    const int m = meas->m, n = h->n_clones_host, d = 24 + 6 * n;
    if (m < 1 || m > RVIO_AUX_MAX_ROWS || (meas->mode != RVIO_AUX_RESIDUAL && meas->mode != RVIO_AUX_VALUE) || (meas->gate != 0 && meas->gate != 1)) return RVIO_ERR_INVALID;
    for (int r = 0; r < m; ++r) {
        if (!std::isfinite(meas->v[r]) || !std::isfinite(meas->sigma[r]) || !(meas->sigma[r] > 0)) { h->err = "rvio_hip_update_aux: a residual is not finite or a sigma is not finite and > 0"; return RVIO_ERR_INVALID; }
        for (int c = 0; c < d; ++c) {
            const double e = meas->H[(size_t)r * d + c];
            if (!std::isfinite(e)) { h->err = "rvio_hip_update_aux: H holds a non-finite value"; return RVIO_ERR_INVALID; }
            const bool rot = c < 3 || (c >= 9 && c < 12) || (c >= 24 && (c - 24) % 6 < 3);
            if (meas->mode == RVIO_AUX_VALUE && rot && e != 0.0) { h->err = "rvio_hip_update_aux: VALUE mode with a non-zero entry in a rotation column of H (xi is 0 there: linearise and use RESIDUAL mode)"; return RVIO_ERR_INVALID; }
        }
    }
    RCCHK(meas_guard(h, "rvio_hip_update_aux"));
    HIPCHK(h, hipSetDevice(h->device));
    // [H (MAX_ROWS x dmax) | v | sigma | one flag per instance], offsets in doubles
    const size_t nH = (size_t)RVIO_AUX_MAX_ROWS * h->dc.dmax, nd = nH + 2 * RVIO_AUX_MAX_ROWS, bytes = nd * sizeof(double) + sizeof(int32_t) * (size_t)h->batch;
    HostStage& s = h->aux.stage;
    RCCHK(stage_acquire(h, s, bytes));
    double* const pin = (double*)s.pin;
    const double* const dev = (const double*)s.dev;
    std::memcpy(pin, meas->H, sizeof(double) * (size_t)m * d);
    std::memcpy(pin + nH, meas->v, sizeof(double) * m);
    std::memcpy(pin + nH + RVIO_AUX_MAX_ROWS, meas->sigma, sizeof(double) * m);
    const int32_t* d_active;
    RCCHK(stage_send(h, s, bytes, instance, &d_active));
    return update_aux_dev(h, m, meas->mode, meas->gate, dev, 0, dev + nH, 0, dev + nH + RVIO_AUX_MAX_ROWS, 0, d_active);
}
// (gamma, applied) of the last rvio_hip_update_aux* call
int rvio_hip_get_aux_diag(rvio_hip* h, int instance, double* gamma, int32_t* applied) {
    if (!h || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    if (!h->aux.diag) { h->err = "rvio_hip_get_aux_diag before the first rvio_hip_update_aux"; return RVIO_ERR_STATE; }
    double g; long long ap;
    RCCHK(read_pair(h, h->aux.diag, instance, &g, &ap));
    if (gamma) *gamma = g;
    if (applied) *applied = (int32_t)ap;
    return RVIO_OK;
}

// ---- the measurement chain: what the device-linearised families (fixes, past-frame fixes, relative poses, map landmarks) share behind their
// argument checks — the rows kernel and the aux launch on the rows it left, once (the plain path, as ever) or, with
// rvio_hip_set_meas_iterations, max_iters times in a fixed sequence on the filter stream (include/rvio_hip.h: the iterated update)
static_assert(sizeof(rvio_meas_iter) == 24 && LP_MEAS_MAX_ITERS == RVIO_MEAS_MAX_ITERS, "include/rvio_hip.h: the iteration record has no padding");
// where a family's rows kernel leaves its rows for the aux launch (strides in doubles) and the (gamma, applied) pairs of its calls
struct MeasRows { const double* H; size_t H_stride; const double* r; size_t r_stride; const double* sigma; size_t sigma_stride; double* pair; };
static int meas_iter_ready(rvio_hip* h) {
    if (h->mi.x0) return RVIO_OK;
    const size_t B = (size_t)h->batch, n_x0 = sizeof(double) * meas_iter_x0_stride(h->dc.nmax) * B, n_dx = sizeof(double) * (size_t)h->dc.dmax * B, n_rec = sizeof(rvio_meas_iter) * B;
    char* blk = nullptr;
    RCCHK(own_dev(h, &blk, meas_iter_block_bytes(h->batch, h->dc.nmax, h->dc.dmax), true));
    h->mi.dx = (double*)(blk + n_x0); h->mi.rec = (rvio_meas_iter*)(blk + n_x0 + n_dx); h->mi.run = (int32_t*)(blk + n_x0 + n_dx + n_rec);
    h->mi.x0 = (double*)blk;
    return RVIO_OK;
}
// one pass of the iterated update on the rows `rw`; d_flags: what the rows kernel of this pass left (pass 0: where to act at all)
static int update_aux_iter_dev(rvio_hip* h, int m, int gate, const MeasRows& rw, const int32_t* d_flags, int pass) {
    const int n = h->n_clones_host;
    const LpLaunch l = aux_iter_launch(n, m, h->batch);
    const size_t w = sizeof(double);
    const AuxIter it = {h->mi.x0, h->mi.dx, h->mi.rec, (int*)h->mi.run, meas_iter_x0_stride(h->dc.nmax), (size_t)h->dc.dmax, pass, h->mi.max_iters - 1, h->mi.tol};
    if (l.kernel == LPK_AUX_ITER4)
        hipLaunchKernelGGL(aux_iter_kernel<4>, lp_grid(l), lp_block(l), l.lds, h->stream, n, h->dc.dmax, m, RVIO_AUX_RESIDUAL, gate, h->x[h->cur], h->P[h->cur], h->d_pose, h->meta,
                           h->slab_bytes, rw.H, rw.H_stride * w, rw.r, rw.r_stride * w, rw.sigma, rw.sigma_stride * w, (const int*)d_flags, rw.pair, it);
    else
        hipLaunchKernelGGL(aux_iter_kernel<16>, lp_grid(l), lp_block(l), l.lds, h->stream, n, h->dc.dmax, m, RVIO_AUX_RESIDUAL, gate, h->x[h->cur], h->P[h->cur], h->d_pose, h->meta,
                           h->slab_bytes, rw.H, rw.H_stride * w, rw.r, rw.r_stride * w, rw.sigma, rw.sigma_stride * w, (const int*)d_flags, rw.pair, it);
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}
// rows(pass, flags) enqueues the family's rows kernel with `flags` as its d_active.  d_own: the flags that kernel writes itself (nullptr: it
// keeps none, the aux launch gets the caller's).  Passes behind the first get the running flags of the block, which the aux launch of the
// pass before cleared for every finished instance.  Ends with the drain of RVIO_PARANOID
extern "C++" template <class Rows>
static int meas_chain(rvio_hip* h, int m, int gate, const MeasRows& rw, const int32_t* d_active, const int32_t* d_own, Rows&& rows) {
    const int K = h->mi.max_iters;
    if (K > 1) RCCHK(meas_iter_ready(h));
    h->mi.last_pair = rw.pair; h->mi.last_iterated = K > 1;
    rows(0, d_active);
    HIPCHK(h, hipGetLastError());
    if (K == 1) {
        RCCHK(update_aux_dev(h, m, RVIO_AUX_RESIDUAL, gate, rw.H, rw.H_stride, rw.r, rw.r_stride, rw.sigma, rw.sigma_stride, d_own ? d_own : d_active, rw.pair));
    } else {
        RCCHK(chol_drop(h, CHOL_FILTER_WAITS));   // (the final pass changes the covariance in place)
        RCCHK(update_aux_iter_dev(h, m, gate, rw, d_own ? d_own : d_active, 0));
        for (int i = 1; i < K; ++i) {
            rows(i, h->mi.run);
            HIPCHK(h, hipGetLastError());
            RCCHK(update_aux_iter_dev(h, m, gate, rw, d_own, i));
        }
    }
    if (paranoid_bits() & PAR_DRAIN) return drain_all(h);
    return RVIO_OK;
}
int rvio_hip_set_meas_iterations(rvio_hip* h, int max_iters, double tol) {
    if (!h) return RVIO_ERR_INVALID;
    if (max_iters < 1 || max_iters > RVIO_MEAS_MAX_ITERS) { h->err = "rvio_hip_set_meas_iterations: max_iters is outside 1 .. RVIO_MEAS_MAX_ITERS"; return RVIO_ERR_INVALID; }
    if (!(std::isfinite(tol) && tol >= 0.0)) { h->err = "rvio_hip_set_meas_iterations: tol is not finite and >= 0"; return RVIO_ERR_INVALID; }
    h->mi.max_iters = max_iters; h->mi.tol = tol;
    return RVIO_OK;
}
int rvio_hip_get_meas_iterations(rvio_hip* h, int* max_iters, double* tol) {
    if (!h) return RVIO_ERR_INVALID;
    if (max_iters) *max_iters = h->mi.max_iters;
    if (tol) *tol = h->mi.tol;
    return RVIO_OK;
}
// waits for the filter stream only
int rvio_hip_get_meas_iter(rvio_hip* h, int instance, rvio_meas_iter* out) {
    if (!h || !out || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    if (!h->mi.last_pair) { h->err = "rvio_hip_get_meas_iter before the first fix, past-fix, rel or map call"; return RVIO_ERR_STATE; }
    double g; long long ap;
    if (h->mi.last_iterated) return read_pair(h, h->mi.last_pair, instance, &g, &ap, out, h->mi.rec + instance, sizeof *out);
    RCCHK(read_pair(h, h->mi.last_pair, instance, &g, &ap));
    out->step = 0.0; out->gamma0 = g; out->iterations = 1; out->converged = 0;
    return RVIO_OK;
}

// ------------------------------------------------------------------ standstill detection (standstill.hip)
static_assert(sizeof(rvio_standstill_config) == 64 && sizeof(rvio_standstill) == 40, "include/rvio_hip.h: the standstill structs have no padding");
void rvio_standstill_config_default(const rvio_config* cfg, rvio_standstill_config* out) {
    if (!cfg || !out) return;
    std::memset(out, 0, sizeof *out);
    // tuning values, not measurements: the discrete-time form of the configured densities; T has mean ~ 6 under them
    out->sigma_a = cfg->sigma_a * std::sqrt(cfg->imu_rate);
    out->sigma_w = cfg->sigma_g * std::sqrt(cfg->imu_rate);
    out->imu_thr = 12.0;
    out->disp_thr_px = 0.5;
    out->sigma_v = 0.05;
    out->sigma_bg = out->sigma_w;
    out->min_pairs = 20; out->bias_rows = 0; out->gate = 1; out->reserved = 0;
}
int rvio_hip_set_standstill(rvio_hip* h, const rvio_standstill_config* c) {
    if (!h) return RVIO_ERR_INVALID;
    if (!c) { h->ss_on = false; return RVIO_OK; }
    auto pos = [](double v) { return std::isfinite(v) && v > 0; };
    const char* bad = nullptr;
    if (!pos(c->sigma_a)) bad = "sigma_a (finite and > 0)";
    else if (!pos(c->sigma_w)) bad = "sigma_w (finite and > 0)";
    else if (!pos(c->imu_thr)) bad = "imu_thr (finite and > 0)";
    else if (std::isnan(c->disp_thr_px)) bad = "disp_thr_px (a number; <= 0: image test off)";
    else if (!pos(c->sigma_v)) bad = "sigma_v (finite and > 0)";
    else if (!pos(c->sigma_bg)) bad = "sigma_bg (finite and > 0)";
    else if (c->min_pairs < 1) bad = "min_pairs (>= 1)";
    else if (c->bias_rows != 0 && c->bias_rows != 1) bad = "bias_rows (0 | 1)";
    else if (c->gate != 0 && c->gate != 1) bad = "gate (0 | 1)";
    if (bad) { h->err = std::string("rvio_hip_set_standstill: bad member ") + bad; return RVIO_ERR_INVALID; }
    h->ss_cfg = *c; h->ss_cfg.reserved = 0;
    h->ss_on = true;
    return RVIO_OK;
}
static int standstill_check(rvio_hip* h) {   // (a handle without a state reports that first, as it always has)
    if (h->has_state && !h->ss_on) { h->err = "rvio_hip_standstill before rvio_hip_set_standstill"; return RVIO_ERR_STATE; }
    return meas_guard(h, "rvio_hip_standstill");
}
// imu_bs: bytes between the instances' samples (0: shared)
static int standstill_dev(rvio_hip* h, const rvio_imu* d_imu, size_t imu_bs, int m, int apply) {
    const size_t B = (size_t)h->batch;
    if (!h->ss_rec) {   // (one block, both events, or nothing: a failure half-way leaves the members null, and the next call starts over)
        const size_t n_rec = sizeof(rvio_standstill) * B, n_diag = 16 * B, n_v = 48 * B, n_H = sizeof(double) * 6 * (size_t)h->dc.dmax, n_sg = 48;
        char* blk = nullptr;
        hipEvent_t ea = nullptr, eb = nullptr;
        int rc = own_dev(h, &blk, n_rec + n_diag + n_v + n_H + n_sg + sizeof(int) * B, true);   // (cleared on the filter stream: whoever reads it first is ordered behind that stream below)
        if (rc == RVIO_OK) rc = own_event(h, &ea, kEvFlags);
        if (rc == RVIO_OK) rc = own_event(h, &eb, kEvFlags);
        if (rc != RVIO_OK) { own_release(h, blk); own_release(h, (void*)ea); return rc; }
        h->ss_rec = (rvio_standstill*)blk; h->ss_diag = (double*)(blk + n_rec); h->ss_v = (double*)(blk + n_rec + n_diag);
        h->ss_H = (double*)(blk + n_rec + n_diag + n_v); h->ss_sigma = (double*)(blk + n_rec + n_diag + n_v + n_H);
        h->ss_active = (int*)(blk + n_rec + n_diag + n_v + n_H + n_sg);
        h->evSSa = ea; h->evSSb = eb;
    }
    // The detector reads hist / hist_len / slot / n_pts, which the refill half of the LAST book-keeping wrote and the NEXT one rewrites: it runs on the
    // stream that ran the last one (stream order on both sides; post_klt_dev covers a next one on another stream), behind the filter stream (bg, ba
    // of the current state, the IMU staging, the cleared block), and the filter stream goes on behind it.  No host wait.
    const bool front = h->front_end;
    const hipStream_t st = (front && h->book_stream) ? h->book_stream : h->stream;
    if (st != h->stream) {
        HIPCHK(h, hipEventRecord(h->evSSa, h->stream));
        HIPCHK(h, hipStreamWaitEvent(st, h->evSSa, 0));
    }
    const int n = h->n_clones_host, rows = h->ss_cfg.bias_rows ? 6 : 3;
    const LpLaunch l = standstill_launch(h->batch);
    hipLaunchKernelGGL(standstill_kernel, lp_grid(l), lp_block(l), l.lds, st, h->dc, (const CamCal*)h->cal, h->t, front ? 1 : 0, (const double*)h->x[h->cur], h->slab_bytes,
                       d_imu, imu_bs, m, h->ss_cfg, n, rows, apply, h->img_count, h->ss_rec, h->ss_active, h->ss_v, h->ss_H, h->ss_sigma, h->ss_diag);
    HIPCHK(h, hipGetLastError());
    if (front) {
        HIPCHK(h, hipEventRecord(h->evSSb, st));
        h->ss_last = st;
    }
    if (st != h->stream) HIPCHK(h, hipStreamWaitEvent(h->stream, h->evSSb, 0));
    if (apply)
        RCCHK(update_aux_dev(h, rows, RVIO_AUX_VALUE, h->ss_cfg.gate, h->ss_H, 0, h->ss_v, 6, h->ss_sigma, 0, (const int32_t*)h->ss_active, h->ss_diag));
    if (paranoid_bits() & PAR_DRAIN) return drain_all(h);
    return RVIO_OK;
}
int rvio_hip_standstill_dev(rvio_hip* h, const rvio_imu* d_imu, int imu_stride, int m, int apply) {
    if (!h || !d_imu || m < 1 || (apply != 0 && apply != 1) || imu_stride < 0 || (imu_stride > 0 && imu_stride < m)) return RVIO_ERR_INVALID;
    RCCHK(standstill_check(h));
    HIPCHK(h, hipSetDevice(h->device));
    return standstill_dev(h, d_imu, (size_t)imu_stride * sizeof(rvio_imu), m, apply);
}
// host buffer: staged through a block of its own (which grows with m), copied on the filter stream — the detector is ordered behind that stream
int rvio_hip_standstill(rvio_hip* h, const rvio_imu* imu, int m, int apply) {
    if (!h || !imu || m < 1 || (apply != 0 && apply != 1)) return RVIO_ERR_INVALID;
    RCCHK(standstill_check(h));
    HIPCHK(h, hipSetDevice(h->device));
    if (m > h->ss_imu_cap) {   // (hipFree waits for what still reads the old block)
        const int cap = std::max(std::max(2 * h->ss_imu_cap, RVIO_HIP_MAX_IMU), (m + 63) & ~63);
        rvio_imu* p = nullptr;
        RCCHK(own_dev(h, &p, sizeof(rvio_imu) * (size_t)cap));
        own_release(h, h->ss_imu);
        h->ss_imu = p; h->ss_imu_cap = cap;
    }
    HIPCHK(h, hipMemcpyAsync(h->ss_imu, imu, sizeof(rvio_imu) * (size_t)m, hipMemcpyHostToDevice, h->stream));
    return standstill_dev(h, h->ss_imu, 0, m, apply);
}
// waits for the filter stream only (that stream waits for the detector wherever it ran)
int rvio_hip_get_standstill(rvio_hip* h, int instance, rvio_standstill* out) {
    if (!h || !out || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    if (!h->ss_rec) { h->err = "rvio_hip_get_standstill before the first rvio_hip_standstill"; return RVIO_ERR_STATE; }
    double g; long long ap;
    RCCHK(read_pair(h, h->ss_diag, instance, &g, &ap, out, h->ss_rec + instance, sizeof *out));
    out->gamma = ap ? g : 0.0;
    if (ap) out->flags |= 8;
    return RVIO_OK;
}

// ------------------------------------------------------------------ absolute fixes (fix_rows.hip)
static_assert(sizeof(rvio_fix) == 128 && sizeof(rvio_fix_diag) == 72, "include/rvio_hip.h: the fix structs have no padding");
static_assert(LP_FIX_ROWS == 6, "launch_plan.h: the rows of a POSE fix");
static const char kFixEntry[] = "rvio_hip_update_fix";   // the state errors of all four entry points name this one
// what the four entry points check of their arguments (the _dev forms have no instance: -1).  kind_max: GRAVITY, or POSE for a past frame
static bool fix_args_ok(const rvio_hip* h, const rvio_fix* fix, int kind, int kind_max, int gate, int instance = -1) {
    return h && fix && kind >= RVIO_FIX_POSITION && kind <= kind_max && (gate == 0 || gate == 1) && instance >= -1 && instance < h->batch;
}
// what the host forms check of a record: every entry the kind uses is finite, its sigmas > 0, its quaternion of unit length
static int fix_record_check(rvio_hip* h, int kind, const rvio_fix* fix) {
    const bool pos = kind == RVIO_FIX_POSITION || kind == RVIO_FIX_POSE, att = kind == RVIO_FIX_ATTITUDE || kind == RVIO_FIX_POSE, vec = pos || kind == RVIO_FIX_GRAVITY;
    auto fin = [](const double* p, int k) { for (int i = 0; i < k; ++i) if (!std::isfinite(p[i])) return false; return true; };
    auto positive = [](const double* p, int k) { for (int i = 0; i < k; ++i) if (!(p[i] > 0)) return false; return true; };
    if ((vec && !(fin(fix->z, 3) && fin(fix->sigma, 3))) || (att && !(fin(fix->z + 3, 4) && fin(fix->sigma + 3, 3))) || (pos && !fin(fix->lever, 3))) {
        h->err = "rvio_hip_update_fix: an entry of z, sigma or lever that this kind uses is not finite"; return RVIO_ERR_INVALID;
    }
    if ((vec && !positive(fix->sigma, 3)) || (att && !positive(fix->sigma + 3, 3))) { h->err = "rvio_hip_update_fix: a sigma that this kind uses is not > 0"; return RVIO_ERR_INVALID; }
    if (att) {
        const double* q = fix->z + 3;
        if (std::fabs(std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) - 1.0) > 1e-6) { h->err = "rvio_hip_update_fix: the quaternion z[3..6] is not of unit length (1e-6)"; return RVIO_ERR_INVALID; }
    }
    return RVIO_OK;
}
// behind the guard: the device, and on the first call the result block — rows, r, sigma, pairs, records — and, for a past frame, the kernel's
// flags (both cleared on the filter stream, where everything that touches them runs)
static int fix_ready(rvio_hip* h, bool past) {
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->fx.H) {
        const size_t B = (size_t)h->batch;
        const size_t n_H = sizeof(double) * LP_FIX_ROWS * (size_t)h->dc.dmax * B, n_r = 48 * B, n_sg = 48 * B, n_pair = 16 * B, n_rec = sizeof(rvio_fix_diag) * B;
        char* blk = nullptr;
        RCCHK(own_dev(h, &blk, n_H + n_r + n_sg + n_pair + n_rec, true));
        h->fx.H = (double*)blk; h->fx.r = (double*)(blk + n_H); h->fx.sigma = (double*)(blk + n_H + n_r); h->fx.pair = (double*)(blk + n_H + n_r + n_sg);
        h->fx.rec = (rvio_fix_diag*)(blk + n_H + n_r + n_sg + n_pair);
    }
    if (!past || h->fp.flag) return RVIO_OK;
    if (h->dc.nmax > LP_FIXP_NMAX) { h->err = "rvio_hip_update_fix_past: the clone window is longer than the chain the kernel holds (launch_plan.h LP_FIXP_NMAX)"; return RVIO_ERR_INVALID; }
    return own_dev(h, &h->fp.flag, sizeof(int32_t) * (size_t)h->batch, true);
}
static size_t fix_H_stride(const rvio_hip* h) { return (size_t)LP_FIX_ROWS * h->dc.dmax; }   // doubles between the instances' rows
// What the three producers share: kind, m and d for the getters, and the measurement chain on the fix block — their rows kernel (`rows`, as
// meas_chain calls it) and the RESIDUAL aux launch on the rows it left, which reads them in stream order and acts where the flags say
extern "C++" template <class Rows>
static int fix_consume(rvio_hip* h, int kind, int gate, const int32_t* d_active, const int32_t* d_own, Rows&& rows) {
    const int m = (kind == RVIO_FIX_POSE || kind == RVIO_REL_POSE) ? 6 : 3;
    h->fx.kind = kind; h->fx.m = m; h->fx.d = 24 + 6 * h->n_clones_host;
    const MeasRows rw = {h->fx.H, fix_H_stride(h), h->fx.r, 6, h->fx.sigma, 6, h->fx.pair};
    return meas_chain(h, m, gate, rw, d_active, d_own, rows);
}
// fix_bs: bytes between the instances' records (0: shared).  The kernel reads x of the current buffer, which the filter stream owns: it runs on
// that stream, no event
static int update_fix_dev(rvio_hip* h, int kind, int gate, const rvio_fix* d_fix, size_t fix_bs, const int32_t* d_active) {
    const LpLaunch l = fix_launch(h->batch);
    return fix_consume(h, kind, gate, d_active, nullptr, [&](int, const int32_t* flags) {
        hipLaunchKernelGGL(fix_rows_kernel, lp_grid(l), lp_block(l), l.lds, h->stream, h->n_clones_host, kind, h->dc.gravity, (const double*)h->x[h->cur], h->slab_bytes, d_fix, fix_bs,
                           (const int*)flags, h->img_count, h->fx.H, fix_H_stride(h) * sizeof(double), h->fx.r, h->fx.sigma, h->fx.rec, h->fx.pair);
    });
}
int rvio_hip_update_fix_dev(rvio_hip* h, int kind, int gate, const rvio_fix* d_fix, size_t fix_stride, const int32_t* d_active) {
    if (!fix_args_ok(h, d_fix, kind, RVIO_FIX_GRAVITY, gate)) return RVIO_ERR_INVALID;
    RCCHK(meas_guard(h, kFixEntry));
    RCCHK(fix_ready(h, false));
    return update_fix_dev(h, kind, gate, d_fix, fix_stride * sizeof(rvio_fix), d_active);
}
// host record: checked here, packed into the pinned block once the copy of the previous call has left it: [one record | one flag per instance]
int rvio_hip_update_fix(rvio_hip* h, int instance, int kind, int gate, const rvio_fix* fix) {
    if (!fix_args_ok(h, fix, kind, RVIO_FIX_GRAVITY, gate, instance)) return RVIO_ERR_INVALID;
    RCCHK(fix_record_check(h, kind, fix));
    RCCHK(meas_guard(h, kFixEntry));
    RCCHK(fix_ready(h, false));
    HostStage& s = h->fx.stage;
    const size_t bytes = sizeof(rvio_fix) + sizeof(int32_t) * (size_t)h->batch;
    RCCHK(stage_acquire(h, s, bytes));
    std::memcpy(s.pin, fix, sizeof *fix);
    const int32_t* d_active;
    RCCHK(stage_send(h, s, bytes, instance, &d_active));
    return update_fix_dev(h, kind, gate, (const rvio_fix*)s.dev, 0, d_active);
}

// ---- past-frame fixes (fix_past.hip): the same consumer, the rows linearised against the pose the window holds for an earlier image
// fix_bs: bytes between the instances' records (0: shared).  On the filter stream like update_fix_dev; the aux launch gets the kernel's own flags
static int update_fix_past_dev(rvio_hip* h, int kind, int gate, const rvio_fix* d_fix, size_t fix_bs, const int32_t* d_age, const double* d_frac, const int32_t* d_active) {
    const LpLaunch l = fix_past_launch(h->batch);
    return fix_consume(h, kind, gate, d_active, h->fp.flag, [&](int, const int32_t* flags) {
        hipLaunchKernelGGL(fix_past_kernel, lp_grid(l), lp_block(l), l.lds, h->stream, h->n_clones_host, kind, (const double*)h->x[h->cur], h->slab_bytes, d_fix, fix_bs, (const int*)d_age, d_frac,
                           (const int*)flags, h->composed_count, h->fx.H, fix_H_stride(h) * sizeof(double), h->fx.r, h->fx.sigma, h->fx.rec, h->fx.pair, (int*)h->fp.flag);
    });
}
int rvio_hip_update_fix_past_dev(rvio_hip* h, int kind, int gate, const rvio_fix* d_fix, size_t fix_stride, const int32_t* d_age, const double* d_frac, const int32_t* d_active) {
    if (!fix_args_ok(h, d_fix, kind, RVIO_FIX_POSE, gate) || !d_age) return RVIO_ERR_INVALID;
    RCCHK(meas_guard(h, kFixEntry));
    RCCHK(fix_ready(h, true));
    return update_fix_past_dev(h, kind, gate, d_fix, fix_stride * sizeof(rvio_fix), d_age, d_frac, d_active);
}
// host record, staged like rvio_hip_update_fix's: [one record | frac | age | flag, each per instance]
int rvio_hip_update_fix_past(rvio_hip* h, int instance, int kind, int gate, int age, double frac, const rvio_fix* fix) {
    if (!fix_args_ok(h, fix, kind, RVIO_FIX_POSE, gate, instance)) return RVIO_ERR_INVALID;
    if (!(frac >= 0.0 && frac < 1.0) || (frac != 0.0 && kind != RVIO_FIX_POSITION)) { h->err = "rvio_hip_update_fix_past: frac is outside [0, 1), or not 0 with a kind other than POSITION"; return RVIO_ERR_INVALID; }
    RCCHK(fix_record_check(h, kind, fix));
    RCCHK(meas_guard(h, kFixEntry));
    if (age < 0 || age + (frac > 0.0 ? 1 : 0) > h->n_clones_host) { h->err = "rvio_hip_update_fix_past: the age (+ 1 with frac > 0) is outside the clone window"; return RVIO_ERR_INVALID; }
    RCCHK(fix_ready(h, true));
    HostStage& s = h->fp.stage;
    const size_t B = (size_t)h->batch, o_frac = sizeof(rvio_fix), o_age = o_frac + sizeof(double) * B, bytes = o_age + 2 * sizeof(int32_t) * B;
    RCCHK(stage_acquire(h, s, bytes));
    std::memcpy(s.pin, fix, sizeof *fix);
    double* fr = (double*)(s.pin + o_frac);
    int32_t* ag = (int32_t*)(s.pin + o_age);
    for (int i = 0; i < h->batch; ++i) { fr[i] = frac; ag[i] = age; }
    const int32_t* d_active;
    RCCHK(stage_send(h, s, bytes, instance, &d_active));
    return update_fix_past_dev(h, kind, gate, (const rvio_fix*)s.dev, 0, (const int32_t*)(s.dev + o_age), (const double*)(s.dev + o_frac), d_active);
}
// ---- relative-pose measurements (rel_rows.hip): the same block, flags and consumer, the rows linearised against the clones between two frames
static_assert(RVIO_REL_POSITION == 16 + RVIO_FIX_POSITION && RVIO_REL_ATTITUDE == 16 + RVIO_FIX_ATTITUDE && RVIO_REL_POSE == 16 + RVIO_FIX_POSE,
              "include/rvio_hip.h: a relative kind is 16 + the fix kind");
static bool rel_args_ok(const rvio_hip* h, const rvio_fix* meas, int kind, int gate, int instance = -1) {
    return h && meas && kind >= RVIO_REL_POSITION && kind <= RVIO_REL_POSE && (gate == 0 || gate == 1) && instance >= -1 && instance < h->batch;
}
// meas_bs: bytes between the instances' records (0: shared).  On the filter stream like update_fix_past_dev; the aux launch gets the kernel's own flags
static int update_rel_dev(rvio_hip* h, int kind, int gate, const rvio_fix* d_meas, size_t meas_bs, const int32_t* d_age_new, const int32_t* d_age_old, const int32_t* d_active) {
    const LpLaunch l = rel_launch(h->batch);
    return fix_consume(h, kind, gate, d_active, h->fp.flag, [&](int, const int32_t* flags) {
        hipLaunchKernelGGL(rel_rows_kernel, lp_grid(l), lp_block(l), l.lds, h->stream, h->n_clones_host, kind, (const double*)h->x[h->cur], h->slab_bytes, d_meas, meas_bs, (const int*)d_age_new,
                           (const int*)d_age_old, (const int*)flags, h->composed_count, h->fx.H, fix_H_stride(h) * sizeof(double), h->fx.r, h->fx.sigma, h->fx.rec, h->fx.pair, (int*)h->fp.flag);
    });
}
int rvio_hip_update_rel_dev(rvio_hip* h, int kind, int gate, const rvio_fix* d_meas, size_t meas_stride, const int32_t* d_age_new, const int32_t* d_age_old, const int32_t* d_active) {
    if (!rel_args_ok(h, d_meas, kind, gate) || !d_age_new || !d_age_old) return RVIO_ERR_INVALID;
    RCCHK(meas_guard(h, "rvio_hip_update_rel"));
    RCCHK(fix_ready(h, true));
    return update_rel_dev(h, kind, gate, d_meas, meas_stride * sizeof(rvio_fix), d_age_new, d_age_old, d_active);
}
// host record, staged like rvio_hip_update_fix_past's: [one record | age_new | age_old | flag, each per instance]
int rvio_hip_update_rel(rvio_hip* h, int instance, int kind, int gate, int age_new, int age_old, const rvio_fix* meas) {
    if (!rel_args_ok(h, meas, kind, gate, instance)) return RVIO_ERR_INVALID;
    RCCHK(fix_record_check(h, kind - RVIO_REL_POSITION, meas));
    RCCHK(meas_guard(h, "rvio_hip_update_rel"));
    if (age_new < 0 || age_old > h->n_clones_host) { h->err = "rvio_hip_update_rel: age_new < 0 or age_old beyond the clone window"; return RVIO_ERR_INVALID; }
    if (age_new >= age_old) { h->err = "rvio_hip_update_rel: age_new is not below age_old (the newer frame first; one frame has no delta)"; return RVIO_ERR_INVALID; }
    RCCHK(fix_ready(h, true));
    HostStage& s = h->rl.stage;
    const size_t B = (size_t)h->batch, o_new = sizeof(rvio_fix), o_old = o_new + sizeof(int32_t) * B, bytes = o_old + 2 * sizeof(int32_t) * B;
    RCCHK(stage_acquire(h, s, bytes));
    std::memcpy(s.pin, meas, sizeof *meas);
    int32_t* an = (int32_t*)(s.pin + o_new);
    int32_t* ao = (int32_t*)(s.pin + o_old);
    for (int i = 0; i < h->batch; ++i) { an[i] = age_new; ao[i] = age_old; }
    const int32_t* d_active;
    RCCHK(stage_send(h, s, bytes, instance, &d_active));
    return update_rel_dev(h, kind, gate, (const rvio_fix*)s.dev, 0, (const int32_t*)(s.dev + o_new), (const int32_t*)(s.dev + o_old), d_active);
}
// host arithmetic only: the age of the frame counted img_count (as rvio_odom.img_count reports it) in the window as it is now
int rvio_hip_frame_age(rvio_hip* h, int img_count, int* age) {
    if (!h || !age) return RVIO_ERR_INVALID;
    const int a = h->composed_count - img_count;
    if (!h->has_state || a < 0 || a > h->n_clones_host) {
        h->err = a < 0 ? "rvio_hip_frame_age: that frame is not composed yet" : "rvio_hip_frame_age: that frame has left the clone window";
        return RVIO_ERR_INVALID;
    }
    *age = a;
    return RVIO_OK;
}
// waits for the filter stream only
int rvio_hip_get_fix(rvio_hip* h, int instance, rvio_fix_diag* out) {
    if (!h || !out || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    if (!h->fx.m) { h->err = "rvio_hip_get_fix before the first rvio_hip_update_fix"; return RVIO_ERR_STATE; }
    double g; long long ap;
    RCCHK(read_pair(h, h->fx.pair, instance, &g, &ap, out, h->fx.rec + instance, sizeof *out));
    out->gamma = g;   // (as compared, also when the gate refused it: by how much is what a caller wants to know then)
    out->applied = ap ? 1 : 0;
    return RVIO_OK;
}
int rvio_hip_get_fix_rows(rvio_hip* h, int instance, int32_t* m, int32_t* d, double* H, double* sigma) {
    if (!h || !m || !d || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    if (!h->fx.m) { h->err = "rvio_hip_get_fix_rows before the first rvio_hip_update_fix"; return RVIO_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    *m = h->fx.m; *d = h->fx.d;
    if (H) HIPCHK(h, hipMemcpyAsync(H, h->fx.H + (size_t)instance * fix_H_stride(h), sizeof(double) * (size_t)h->fx.m * h->fx.d, hipMemcpyDeviceToHost, h->stream));
    if (sigma) HIPCHK(h, hipMemcpyAsync(sigma, h->fx.sigma + 6 * (size_t)instance, sizeof(double) * (size_t)h->fx.m, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}

// ---- map landmarks (map_rows.hip): pixel observations of known world points; a block, flags and getters of their own, the same guard, staging,
// pair read-back and aux launch
static_assert(sizeof(rvio_map_obs) == 48 && sizeof(rvio_map_point) == 40 && sizeof(rvio_map_diag) == 32, "include/rvio_hip.h: the map structs have no padding");
static_assert(LP_MAP_POINTS == RVIO_MAP_MAX_POINTS && LP_MAP_ROWS == RVIO_AUX_MAX_ROWS, "launch_plan.h: the points and rows of a map call");
static const char kMapEntry[] = "rvio_hip_update_map";
// what both entry points check of their arguments (the _dev form has no instance: -1): the cause, or nullptr
static const char* map_args_bad(const rvio_hip* h, const rvio_map_obs* obs, int units, int gate, int gate_each, int n, int instance = -1) {
    if (!h) return "NULL handle";
    if (!obs) return "NULL observations";
    if (units != RVIO_MAP_NORMALISED && units != RVIO_MAP_PIXELS) return "units is neither RVIO_MAP_NORMALISED nor RVIO_MAP_PIXELS";
    if ((gate != 0 && gate != 1) || (gate_each != 0 && gate_each != 1)) return "gate and gate_each are 0 or 1";
    if (n < 1 || n > RVIO_MAP_MAX_POINTS) return "the number of observations is outside 1 .. RVIO_MAP_MAX_POINTS";
    if (instance < -1 || instance >= h->batch) return "instance out of range";
    return nullptr;
}
static int map_refuse(rvio_hip* h, const char* why) {
    if (h) h->err = std::string(kMapEntry) + ": " + why;
    return RVIO_ERR_INVALID;
}
// behind the guard: the device, and on the first call the block (cleared on the filter stream, where everything that touches it runs)
static int map_ready(rvio_hip* h) {
    HIPCHK(h, hipSetDevice(h->device));
    if (h->mp.H) return RVIO_OK;
    if (h->dc.nmax > LP_FIXP_NMAX) { h->err = "rvio_hip_update_map: the clone window is longer than the chain the kernel holds (launch_plan.h LP_FIXP_NMAX)"; return RVIO_ERR_INVALID; }
    const size_t B = (size_t)h->batch;
    const size_t n_H = sizeof(double) * map_H_stride(h->dc.dmax) * B, n_r = sizeof(double) * LP_MAP_ROWS * B, n_pair = 16 * B, n_rec = sizeof(rvio_map_diag) * B,
                 n_pts = sizeof(rvio_map_point) * LP_MAP_POINTS * B;
    char* blk = nullptr;
    RCCHK(own_dev(h, &blk, map_block_bytes(h->batch, h->dc.dmax), true));
    h->mp.r = (double*)(blk + n_H); h->mp.sigma = (double*)(blk + n_H + n_r); h->mp.pair = (double*)(blk + n_H + 2 * n_r);
    h->mp.rec = (rvio_map_diag*)(blk + n_H + 2 * n_r + n_pair); h->mp.pts = (rvio_map_point*)(blk + n_H + 2 * n_r + n_pair + n_rec);
    h->mp.flag = (int32_t*)(blk + n_H + 2 * n_r + n_pair + n_rec + n_pts);
    h->mp.H = (double*)blk;
    return RVIO_OK;
}
// obs_bs: bytes between the instances' records (0: shared).  The kernel reads x and P of the current buffer, which the filter stream owns: it
// runs on that stream, no event; the aux launch gets the kernel's own flags
static int update_map_dev(rvio_hip* h, int units, int gate, int gate_each, int n_max, const rvio_map_obs* d_obs, size_t obs_bs, const int32_t* d_count,
                          const int32_t* d_age, const int32_t* d_active) {
    const LpLaunch l = map_launch(h->batch);
    const size_t Hs = map_H_stride(h->dc.dmax);
    h->mp.m = 2 * n_max; h->mp.d = 24 + 6 * h->n_clones_host;
    const MeasRows rw = {h->mp.H, Hs, h->mp.r, LP_MAP_ROWS, h->mp.sigma, LP_MAP_ROWS, h->mp.pair};
    return meas_chain(h, 2 * n_max, gate, rw, d_active, h->mp.flag, [&](int pass, const int32_t* flags) {
        hipLaunchKernelGGL(map_rows_kernel, lp_grid(l), lp_block(l), l.lds, h->stream, h->dc, (const CamCal*)h->cal, h->n_clones_host, h->dc.dmax, units, gate_each, n_max,
                           (const double*)h->x[h->cur], (const double*)h->P[h->cur], h->slab_bytes, d_obs, obs_bs, (const int*)d_count, (const int*)d_age, (const int*)flags,
                           h->composed_count, h->mp.H, Hs * sizeof(double), h->mp.r, h->mp.sigma, h->mp.rec, h->mp.pts, h->mp.pair, (int*)h->mp.flag, pass);
    });
}
int rvio_hip_update_map_dev(rvio_hip* h, int units, int gate, int gate_each, int n_max, const rvio_map_obs* d_obs, size_t obs_stride, const int32_t* d_count,
                            const int32_t* d_age, const int32_t* d_active) {
    if (const char* why = map_args_bad(h, d_obs, units, gate, gate_each, n_max)) return map_refuse(h, why);
    if (!d_age) return map_refuse(h, "NULL d_age");
    if (obs_stride && obs_stride < (size_t)n_max) return map_refuse(h, "obs_stride is below n_max and not 0");
    RCCHK(meas_guard(h, kMapEntry));
    RCCHK(map_ready(h));
    return update_map_dev(h, units, gate, gate_each, n_max, d_obs, obs_stride * sizeof(rvio_map_obs), d_count, d_age, d_active);
}
// host records, staged like rvio_hip_update_fix_past's: [RVIO_MAP_MAX_POINTS records | age | flag, each per instance]
int rvio_hip_update_map(rvio_hip* h, int instance, int units, int gate, int gate_each, int age, int n_obs, const rvio_map_obs* obs) {
    if (const char* why = map_args_bad(h, obs, units, gate, gate_each, n_obs, instance)) return map_refuse(h, why);
    for (int j = 0; j < n_obs; ++j) {
        const rvio_map_obs& o = obs[j];
        if (!(std::isfinite(o.p_w[0]) && std::isfinite(o.p_w[1]) && std::isfinite(o.p_w[2]) && std::isfinite(o.uv[0]) && std::isfinite(o.uv[1]) && std::isfinite(o.sigma))) {
            h->err = "rvio_hip_update_map: a member of an observation is not finite"; return RVIO_ERR_INVALID;
        }
        if (!(o.sigma > 0)) { h->err = "rvio_hip_update_map: a sigma is not > 0"; return RVIO_ERR_INVALID; }
    }
    RCCHK(meas_guard(h, kMapEntry));
    if (age < 0 || age > h->n_clones_host) { h->err = "rvio_hip_update_map: the age is outside the clone window"; return RVIO_ERR_INVALID; }
    RCCHK(map_ready(h));
    HostStage& s = h->mp.stage;
    const size_t B = (size_t)h->batch, o_age = sizeof(rvio_map_obs) * RVIO_MAP_MAX_POINTS, bytes = o_age + 2 * sizeof(int32_t) * B;
    RCCHK(stage_acquire(h, s, bytes));
    std::memcpy(s.pin, obs, sizeof(rvio_map_obs) * (size_t)n_obs);
    int32_t* ag = (int32_t*)(s.pin + o_age);
    for (int i = 0; i < h->batch; ++i) ag[i] = age;
    const int32_t* d_active;
    RCCHK(stage_send(h, s, bytes, instance, &d_active));
    return update_map_dev(h, units, gate, gate_each, n_obs, (const rvio_map_obs*)s.dev, 0, nullptr, (const int32_t*)(s.dev + o_age), d_active);
}
// wait for the filter stream only
int rvio_hip_get_map(rvio_hip* h, int instance, rvio_map_diag* out, rvio_map_point* pts) {
    if (!h || !out || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    if (!h->mp.m) { h->err = "rvio_hip_get_map before the first rvio_hip_update_map"; return RVIO_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    if (pts) HIPCHK(h, hipMemcpyAsync(pts, h->mp.pts + LP_MAP_POINTS * (size_t)instance, sizeof(rvio_map_point) * LP_MAP_POINTS, hipMemcpyDeviceToHost, h->stream));
    double g; long long ap;
    RCCHK(read_pair(h, h->mp.pair, instance, &g, &ap, out, h->mp.rec + instance, sizeof *out));
    out->gamma = g;
    out->applied = ap ? 1 : 0;
    return RVIO_OK;
}
int rvio_hip_get_map_rows(rvio_hip* h, int instance, int32_t* m, int32_t* d, double* H, double* r, double* sigma) {
    if (!h || !m || !d || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    if (!h->mp.m) { h->err = "rvio_hip_get_map_rows before the first rvio_hip_update_map"; return RVIO_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    *m = h->mp.m; *d = h->mp.d;
    const size_t rows = (size_t)h->mp.m;
    if (H) HIPCHK(h, hipMemcpyAsync(H, h->mp.H + (size_t)instance * map_H_stride(h->dc.dmax), sizeof(double) * rows * h->mp.d, hipMemcpyDeviceToHost, h->stream));
    if (r) HIPCHK(h, hipMemcpyAsync(r, h->mp.r + LP_MAP_ROWS * (size_t)instance, sizeof(double) * rows, hipMemcpyDeviceToHost, h->stream));
    if (sigma) HIPCHK(h, hipMemcpyAsync(sigma, h->mp.sigma + LP_MAP_ROWS * (size_t)instance, sizeof(double) * rows, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}

// ------------------------------------------------------------------ S1 + S2
static int augment_compose_dev(rvio_hip* h, int do_augment) {
    const DevCfg& d = h->dc;
    const int c = h->cur, o = c ^ 1;
    // one stream: width (one entry per thread, ~29 workgroups); a batch: every workgroup builds Vk first (a serial section of one thread),
    // so few fat workgroups per instance (the chip is full anyway)
    const int cg = 1 + (h->batch >= 128 ? 4 : std::max(1, std::min(64, (d.dmax * d.dmax + 255) / 256)));
    unsigned long long* done = nullptr;
    if (h->batch == 1) { done = &h->stage_sync->aug; h->stage_tgt.aug += (unsigned long long)cg; }
    // the clone block changes (window slide / new clone).  (A factor still in flight here: a frame without an update never consumed it)
    RCCHK(chol_drop(h, CHOL_FILTER_WAITS));
    hipLaunchKernelGGL(augcomp_kernel2, dim3(cg, 1, h->batch), dim3(256), 0, h->stream, d, h->n_clones_host, do_augment, h->x[c], h->P[c], h->x[o], h->P[o], h->d_pose,
                       h->slab_bytes, done);
    HIPCHK(h, hipGetLastError());
    h->cur = o;
    if (do_augment && h->n_clones_host < d.nmax) h->n_clones_host++;
    h->composed_count = h->img_count;
    // Long windows (6n > 96, solve in its split form): Pcc = L L^T of the NEXT update is known from here on — propagation leaves the clone block
    // alone — so the factor starts now on a stream of its own and runs beside propagate, the wait for the tracker and the per-feature stage; the
    // solve's first product waits for it (launch_solve).  ~35 us at 6n = 120, ~95 us at 6n = 180 off the filter chain.
    if (forms_at(h, h->n_clones_host).chol == LPC_QUEUE && !profiler_serialises()) {
        HIPCHK(h, hipEventRecord(h->evA, h->stream));
        HIPCHK(h, hipStreamWaitEvent(h->stream_l, h->evA, 0));
        launch_s9_chol(h, h->plan.solve9_nt, h->n_clones_host, h->P[h->cur], h->stream_l);
        HIPCHK(h, hipEventRecord(h->evL, h->stream_l));
        chol_queued(h);
    }
    // the odometry record of this frame: behind evA (the run-ahead factor above starts when it did before), on the filter stream (whatever waits
    // for "the filter has finished" through an event waits for the record too; the device-side counter augcomp_kernel2 bumps guards the hand-over
    // tables, which the record does not read).  It reads x / P / pose as augcomp_kernel2 left them; the next writer of either is the next frame's
    // propagate, behind it on this stream.
    if (h->odom.on) {
        h->odom.seq++;
        launch_odom(h, h->odom.slot(h->odom.seq, h->batch), h->odom.seq);
        HIPCHK(h, hipGetLastError());
    }
    // the smoothed record behind it, same stream, same inputs: the frame smo_lag images back, once the window reaches that far
    if (h->smo.on && h->n_clones_host >= h->smo_lag) {
        h->smo.seq++;
        launch_window_pose(h, h->batch, h->x[h->cur], h->P[h->cur], h->smo_lag, 1, h->smo.seq, h->smo.slot(h->smo.seq, h->batch), 1);
        HIPCHK(h, hipGetLastError());
    }
    // the edge record behind it, likewise: the pair (edg_new, edg_old), once the window reaches the older frame
    if (h->edg.on && h->n_clones_host >= h->edg_old) {
        h->edg.seq++;
        launch_window_edge(h, h->batch, h->x[h->cur], h->P[h->cur], 1, nullptr, nullptr, h->edg_new, h->edg_old, h->edg.seq, h->edg.slot(h->edg.seq, h->batch), 1);
        HIPCHK(h, hipGetLastError());
    }
    return RVIO_OK;
}
int rvio_hip_augment_compose(rvio_hip* h, int do_augment) {
    if (!h) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    return augment_compose_dev(h, do_augment);
}

// ------------------------------------------------------------------ T7 detector (device), allocated on first use
static int detector_check(rvio_hip* h) {
    const int cell1 = (int)std::nearbyint((double)h->cfg.min_dist);
    if (cell1 < 1) { h->err = "Tracker.nMinDist < 1 is not supported by the device detector"; return RVIO_ERR_UNSUPPORTED; }
    const int spw = (int)std::floor(.5 * h->cfg.min_dist);   // cornerSubPix half-window, FeatureDetector.cc:68
    if (spw < 1 || spw > 63) { h->err = "device cornerSubPix takes half-windows 1..63 (2 <= Tracker.nMinDist < 128)"; return RVIO_ERR_UNSUPPORTED; }
    return RVIO_OK;
}
static int detector_alloc_set(rvio_hip* h, DetDev& q) {   // the scratch of ONE detector in flight
    const DevCfg& d = h->dc;
    const int cell1 = (int)std::nearbyint((double)h->cfg.min_dist), cell2 = (int)std::nearbyint((double)(2.f * h->cfg.min_dist));
    const size_t npx = (size_t)d.W * d.H;
    q.W = d.W; q.H = d.H; q.F = d.F; q.min_dist = h->cfg.min_dist; q.quality = (double)h->cfg.qual_lvl;
    q.max_cells = ((d.W + cell1 - 1) / cell1) * ((d.H + cell1 - 1) / cell1);
    q.first = h->t.first;
    q.eig = nullptr;   // (the pipeline keeps the min-eigenvalue map in LDS; rvio_hip_get_corners(eig) allocates ONE map per handle on first use)
    DALLOC(h, q.maxkey, 1); DALLOC(h, q.counters, 4); DALLOC(h, q.cell_cnt, (size_t)q.max_cells);
    DALLOC(h, q.cell_ent, (size_t)(d.W + cell2) * (d.H + cell2)); DALLOC(h, q.cell_ci, (size_t)(d.W + cell2) * (d.H + cell2));
    q.n_cap = (int)std::min(npx, (size_t)16384);
    DALLOC(h, q.nb, (size_t)q.n_cap * DET_NBCAP); DALLOC(h, q.nb_cnt, (size_t)q.n_cap);
    DALLOC(h, q.prov, npx); DALLOC(h, q.cand, npx); DALLOC(h, q.acc, npx); DALLOC(h, q.state, npx);
    DALLOC(h, q.raw_xy, (size_t)2 * d.F);
    return RVIO_OK;
}
static int detector_alloc(rvio_hip* h) {   // DALLOCs only (runs twice for a slab)
    const DevCfg& d = h->dc;
    int rc = RVIO_OK;
    for (int k = 0; k < h->plan.n_ic; ++k) if ((rc = detector_alloc_set(h, h->dets[k])) != RVIO_OK) return rc;
    for (int k = h->plan.n_ic; k < rvio_hip::kIC; ++k) h->dets[k] = h->dets[0];
    DALLOC(h, h->det_xy2[0], (size_t)2 * d.F); DALLOC(h, h->det_xy2[1], (size_t)2 * d.F); DALLOC(h, h->det_xy2[2], (size_t)2 * d.F);
    DALLOC(h, h->det_nout, 3);
    float* mask = nullptr;
    const size_t mside = (size_t)std::max(31, 2 * (int)std::floor(.5 * h->cfg.min_dist) + 1);
    DALLOC(h, mask, mside * mside);
    for (DetDev* q : {&h->dets[0], &h->dets[1], &h->dets[2]}) { q->xy = h->det_xy2[0]; q->n_out = h->det_nout; q->spmask = mask; q->sp_win = (int)std::floor(.5 * h->cfg.min_dist); }
    return RVIO_OK;
}
static int detector_init(rvio_hip* h) {
    if (h->det_ready) return RVIO_OK;
    int rc = detector_check(h);
    if (rc != RVIO_OK) return rc;
    if (!h->det_in_slab && (rc = detector_alloc(h)) != RVIO_OK) return rc;
    DetDev& q = h->dets[0];
    // cornerSubPix window (cornersubpix.cpp): float expf on the host, so that device and oracle share glibc's values
    const int spw = q.sp_win, spww = 2 * spw + 1;
    std::vector<float> hm((size_t)spww * spww);
    for (int i = 0; i < spww; ++i) {
        const float y = (float)(i - spw) / (float)spw;
        const float vy = std::exp(-y * y);
        for (int j = 0; j < spww; ++j) { const float x = (float)(j - spw) / (float)spw; hm[(size_t)i * spww + j] = (float)(vy * std::exp(-x * x)); }
    }
    HIPCHK(h, hipMemcpyAsync(const_cast<float*>(q.spmask), hm.data(), sizeof(float) * hm.size(), hipMemcpyHostToDevice, h->stream));   // one copy, shared by all instances
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (hm is a local)
    if (spw > 15) {   // (the limit from the kernel file's own formula; front_forms() hands the launch launch_plan.h's copy of it)
        if (lp_subpix_wide_lds(spw) != subpix_wide_lds(spw)) { h->err = "launch_plan.h: lp_subpix_wide_lds disagrees with detector.hip"; return RVIO_ERR_UNSUPPORTED; }
        HIPCHK(h, lds_attr((const void*)subpix_wide_kernel, (int)subpix_wide_lds(spw)));
    }
    std::vector<int> minkey((size_t)h->batch, (int)0x80000000);
    for (DetDev* qq : {&h->dets[0], &h->dets[1], &h->dets[2]})
        HIPCHK(h, hipMemcpy2DAsync(qq->maxkey, h->slab_bytes ? h->slab_bytes : sizeof(int), minkey.data(), sizeof(int), sizeof(int), (size_t)(h->det_in_slab ? h->batch : 1),
                                   hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, lds_attr((const void*)neigh_kernel, (int)NEIGH_LDS));
    HIPCHK(h, lds_attr((const void*)greedy_kernel, (int)GREEDY_LDS));
    h->det_ready = true;
    return RVIO_OK;
}
// Front-end sequencing.  What a call launches and how its chains are ordered against each other is decided in ONE place, front_forms()
// (launch_plan.h): the mode (plain | run-ahead, device-side counters | stream events), every wait and signal between the queues, the stream
// role of every stage and the form of every kernel — the reasons stand there, next to the rule.  A call computes that value once (call_forms)
// and passes it down by const&; the stages below switch on it and keep the stream and event OBJECTS.
static DetDev det_view(const rvio_hip* h, int det_set, int dslot) {
    DetDev q = h->dets[det_set];
    q.xy = h->det_xy2[dslot]; q.n_out = h->det_nout + dslot;
    return q;
}
// a stream role of front_forms() -> the handle's stream (ic: the image chain of the call, for LPR_IMAGE)
static hipStream_t stream_of(const rvio_hip* h, LpStream role, int ic) {
    switch (role) {
    case LPR_FILTER: break;
    case LPR_TRACKER: return h->stream_t;
    case LPR_SIDE: return h->stream_d;
    case LPR_IMAGE: return ic == 0 ? h->stream_t : h->stream_c;
    }
    return h->stream;
}
// mbIsTheFirstImage: the host sees it in the mirror book-keeping writes, until it has gone to 0 in every instance (cached: it never comes back).  The
// entry points refresh the cache in front of a call that runs the detector; call_forms() below only reads it
static void refresh_first_cleared(rvio_hip* h) {
    if (h->first_cleared) return;
    bool all0 = true;
    for (int i = 0; i < h->batch && all0; ++i) all0 = ((volatile int*)h->first_mirror)[i] == 0;
    h->first_cleared = all0;
}
// rvio_pixel_format: bit 4 = 16-bit samples, bit 5 = Bayer mosaic (low bits: the pattern), else the five 8-bit formats
static bool pix_is16(int fmt) { return (fmt & 16) != 0; }
static bool pix_is_bayer(int fmt) { return (fmt & 32) != 0; }
static bool pix_known(int fmt) {
    if (fmt < 0 || (fmt & ~63)) return false;
    return pix_is_bayer(fmt) ? (fmt & 15) <= 3 : (fmt & 15) <= 4;
}
static int pix_samples(int fmt) {   // samples per pixel
    if (pix_is_bayer(fmt)) return 1;
    const int k = fmt & 15;
    return k == 0 ? 1 : k <= 2 ? 3 : 4;
}
static int pix_bytes(int fmt) { return pix_samples(fmt) * (pix_is16(fmt) ? 2 : 1); }   // bytes per pixel as staged
// what every image entry point checks of the caller's image: the row holds W pixels; 16-bit samples lie on even addresses (d_img: a DEVICE address,
// nullptr for a host buffer, which is staged row by row)
static int check_image(rvio_hip* h, const void* d_img, int stride, size_t img_stride) {
    if (stride < h->dc.W * h->pix_ch) return RVIO_ERR_INVALID;
    if (pix_is16(h->pix_fmt) && ((stride & 1) || (img_stride & 1) || ((uintptr_t)d_img & 1))) {
        h->err = "a 16-bit image format needs an even row stride, instance stride and device address";
        return RVIO_ERR_INVALID;
    }
    return RVIO_OK;
}
// The forms of ONE front-end call: the only place the mode of a call is derived.  img / stride / img_bs: the caller's image (nullptr: none)
static FrontForms call_forms(const rvio_hip* h, bool piped_call, bool have_corner_list, const uint8_t* img, int stride, size_t img_bs) {
    const DevCfg& d = h->dc;
    FrontIn in;
    in.batch = h->batch; in.throughput = h->wide_px;
    in.W = d.W; in.H = d.H; in.F = d.F; in.nmax = d.nmax;
    in.equalizer = h->cfg.enable_equalizer != 0;
    in.cl_tx = h->cl_tx; in.cl_ty = h->cl_ty; in.cl_tw = h->cl_tw; in.cl_th = h->cl_th;
    in.sp_win = (int)std::floor(.5 * h->cfg.min_dist);   // cornerSubPix half-window, FeatureDetector.cc:68
    in.channels = pix_samples(h->pix_fmt); in.bits = pix_is16(h->pix_fmt) ? 16 : 8; in.bayer = pix_is_bayer(h->pix_fmt);
    in.piped_call = piped_call; in.have_corner_list = have_corner_list; in.frame_no = h->frame_no; in.first_cleared = h->first_cleared;
    in.src_dword = stride % 4 == 0 && ((uintptr_t)img & 3) == 0 && img_bs % 4 == 0;
    in.no_runahead = no_runahead(); in.no_device_polls = no_device_polls();
    in.own_queues = h->private_queues && !h->queues_shared && !h->extra_queues;
    return front_forms(h->plan, in);
}
static int detect_dev(rvio_hip* h, const FrontForms& f, const uint8_t* img, int stride, size_t src_bs) {
    const size_t bs = h->slab_bytes;
    const unsigned B = (unsigned)h->batch;
    const DetDev q = det_view(h, f.det_set, f.dslot);
    const hipStream_t ds = stream_of(h, f.image, f.ic);
    switch (f.det_first) {
    case LPDF_NONE: break;
    case LPDF_STRIP:
        hipLaunchKernelGGL(mineig_nms_strip_kernel, lp_grid(f.det_first_l), lp_block(f.det_first_l), 0, ds, img, stride, q, src_bs, bs);
        break;
    case LPDF_TILE:
        hipLaunchKernelGGL(mineig_nms_kernel, lp_grid(f.det_first_l), lp_block(f.det_first_l), 0, ds, img, stride, q, src_bs, bs, (int)h->frame_no,
                           f.det_folds_signal ? &h->stage_sync->pyr[f.ic] : (unsigned long long*)nullptr);   // what this frame's klt_kernel3 polls, if it polls (build_pyramid_dev)
        break;
    }
    if (f.wait_first_flag) HIPCHK(h, hipStreamWaitEvent(ds, h->evT[(h->frame_no - 1) & 3], 0));   // the threshold pass reads mbIsTheFirstImage (cell size) as book-keeping(k-1) left it
    hipLaunchKernelGGL(nms_threshold_kernel, dim3(16, 1, B), dim3(NMS_T), 0, ds, q, bs);
    hipLaunchKernelGGL(neigh_kernel, lp_grid(f.neigh_l), lp_block(f.neigh_l), f.neigh_l.lds, ds, q, bs);
    hipLaunchKernelGGL(greedy_kernel, lp_grid(f.greedy_l), lp_block(f.greedy_l), f.greedy_l.lds, ds, q, bs);
    launch_subpix(h, f, q, img, stride, src_bs, (int)h->frame_no, ds);
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}

// ------------------------------------------------------------------ gray conversion (Tracker.cc:182-196)
// B interleaved images -> B packed gray images (instance stride W * H) on `st`, in the form f names
static void launch_gray(rvio_hip* h, const FrontForms& f, const uint8_t* src, int stride, size_t src_bs, uint8_t* dst, hipStream_t st) {
    const DevCfg& d = h->dc;
    const int bgr = (!pix_is_bayer(h->pix_fmt) && ((h->pix_fmt & 15) == RVIO_PIX_BGR8 || (h->pix_fmt & 15) == RVIO_PIX_BGRA8)) ? 1 : 0;
    const int pat = h->pix_fmt & 3;   // of a mosaic: RGGB, BGGR, GBRG, GRBG
    const size_t bs = (size_t)d.W * d.H;
    const dim3 g = lp_grid(f.gray_l), b = lp_block(f.gray_l);
    switch (f.gray) {
    case LPGR_NONE: break;
    case LPGR_DWORD3: hipLaunchKernelGGL(gray_kernel4<3>, g, b, 0, st, src, d.W, d.H, stride, bgr, dst, src_bs, bs); break;
    case LPGR_BYTE3: hipLaunchKernelGGL(gray_kernel<3>, g, b, 0, st, src, d.W, d.H, stride, bgr, dst, src_bs, bs); break;
    case LPGR_DWORD4: hipLaunchKernelGGL(gray_kernel4<4>, g, b, 0, st, src, d.W, d.H, stride, bgr, dst, src_bs, bs); break;
    case LPGR_BYTE4: hipLaunchKernelGGL(gray_kernel<4>, g, b, 0, st, src, d.W, d.H, stride, bgr, dst, src_bs, bs); break;
    case LPGR_W16_1: hipLaunchKernelGGL(raw16_kernel4<1>, g, b, 0, st, src, d.W, d.H, stride, bgr, dst, src_bs, bs); break;
    case LPGR_P16_1: hipLaunchKernelGGL(raw16_kernel<1>, g, b, 0, st, src, d.W, d.H, stride, bgr, dst, src_bs, bs); break;
    case LPGR_W16_3: hipLaunchKernelGGL(raw16_kernel4<3>, g, b, 0, st, src, d.W, d.H, stride, bgr, dst, src_bs, bs); break;
    case LPGR_P16_3: hipLaunchKernelGGL(raw16_kernel<3>, g, b, 0, st, src, d.W, d.H, stride, bgr, dst, src_bs, bs); break;
    case LPGR_W16_4: hipLaunchKernelGGL(raw16_kernel4<4>, g, b, 0, st, src, d.W, d.H, stride, bgr, dst, src_bs, bs); break;
    case LPGR_P16_4: hipLaunchKernelGGL(raw16_kernel<4>, g, b, 0, st, src, d.W, d.H, stride, bgr, dst, src_bs, bs); break;
    case LPGR_BAYER8_W: hipLaunchKernelGGL(bayer_kernel4<uint8_t>, g, b, 0, st, src, d.W, d.H, stride, pat, dst, src_bs, bs); break;
    case LPGR_BAYER8_P: hipLaunchKernelGGL(bayer_kernel<uint8_t>, g, b, 0, st, src, d.W, d.H, stride, pat, dst, src_bs, bs); break;
    case LPGR_BAYER16_W: hipLaunchKernelGGL(bayer_kernel4<uint16_t>, g, b, 0, st, src, d.W, d.H, stride, pat, dst, src_bs, bs); break;
    case LPGR_BAYER16_P: hipLaunchKernelGGL(bayer_kernel<uint16_t>, g, b, 0, st, src, d.W, d.H, stride, pat, dst, src_bs, bs); break;
    }
}
int rvio_hip_get_image_format(const rvio_hip* h) { return h ? h->pix_fmt : RVIO_ERR_INVALID; }
int rvio_hip_set_image_format(rvio_hip* h, int format) {
    if (!h) return RVIO_ERR_INVALID;
    if (!pix_known(format)) { h->err = "unknown image format"; return RVIO_ERR_INVALID; }
    if (format != RVIO_PIX_MONO8 && !h->front_end) { h->err = "this batch handle was created without its front end: it takes no image"; return RVIO_ERR_UNSUPPORTED; }
    if (format == h->pix_fmt) return RVIO_OK;
    if (pix_is_bayer(format) && (h->dc.W < 3 || h->dc.H < 3)) { h->err = "a Bayer format needs an image of at least 3 x 3 pixels"; return RVIO_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    { const int rc = drain_all(h); if (rc != RVIO_OK) return rc; }   // nothing in flight reads the staging or a gray buffer any more
    const int ch = pix_bytes(format);   // bytes per pixel as staged
    const size_t npx = (size_t)h->dc.W * h->dc.H;
    if (format != RVIO_PIX_MONO8 && !h->d_gray[0]) {   // first converting format: the gray buffers of every instance
        uint8_t* p = nullptr;
        RCCHK(own_dev(h, &p, 4 * npx * (size_t)h->batch, true));
        for (int k = 0; k < 4; ++k) h->d_gray[k] = p + (size_t)k * npx * h->batch;
    }
    if (npx * ch > h->img_cap) {     // the staging of the host-buffer entry points grows to the interleaved image (the old blocks stay where they were, as in ensure_imu_capacity)
        auto grow = [&](uint8_t** q) { return own_dev(h, q, npx * ch); };
        int rc = grow(&h->d_img);
        for (int k = 0; k < 2 && rc == RVIO_OK; ++k) if (h->hb_img[k]) rc = grow(&h->hb_img[k]);
        if (rc != RVIO_OK) return rc;
        h->img_cap = npx * ch;
    }
    if (ch != h->pix_ch) drop_pin_ring(h);   // rvio_hip_frame lays the pinned ring out again (the image slot changes size)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->pix_fmt = format; h->pix_ch = ch;
    h->last.gray_src = nullptr;
    return RVIO_OK;
}

// ------------------------------------------------------------------ T1..T6
// Per-call values one stage hands to the next (no handle state: a call that fails half-way leaves nothing behind).
struct KltWait { const unsigned long long* counter = nullptr; unsigned long long target = 0; };   // what this call's klt_kernel3 polls (nullptr: nothing)
// what run-ahead book-keeping waits for before it rewrites the hand-over table — the filter that read it last: an event in front of it, or the filter
// chain's counter (stage_sync->aug) reaching `target` inside it
struct BookWait { hipEvent_t evt = nullptr; bool dev = false; unsigned long long target = 0; };
// what book-keeping left for the filter of this frame: it starts behind stage_gate_kernel (gate, gate_target), else behind an event — evH recorded behind
// the hand-over half (handover_evt), else the caller's own behind all of book-keeping
struct BookOut { bool gate = false; unsigned long long gate_target = 0; bool handover_evt = false; };

static int build_pyramid_dev(rvio_hip* h, const FrontForms& f, const uint8_t* d_img, int stride, int b, KltWait* klt) {
    const DevCfg& d = h->dc;
    PyrDev& p = h->pyr[b];
    const size_t bs = h->slab_bytes;
    size_t src_bs = h->img_bs;       // the caller's images: instance stride of the call in progress
    const hipStream_t is = stream_of(h, f.image, f.ic);
    auto launch_pyramid = [&](hipStream_t st) {
        PyrDev pv = p;
        const bool own = f.pyramid == LPP_OWN;   // d_img is the handle's equalised image: level 0 without a copy
        if (own) { h->pyr[b].img[0] = d_img; pv.img[0] = d_img; }
        hipLaunchKernelGGL(pyramid_kernel, lp_grid(f.pyramid_l), lp_block(f.pyramid_l), 0, st, d_img, stride, pv, d.levels, own ? 0 : 1, src_bs, bs);
    };
    if (f.wait_book_k3) HIPCHK(h, hipStreamWaitEvent(is, h->evT[(h->frame_no - 3) & 3], 0));
    if (f.gray != LPGR_NONE) {   // colour camera: "Convert to gray scale", Tracker.cc:182-196 — the first launch of the image chain; every later reader sees the handle's gray image
        // Four gray buffers in rotation (one step per image, so slot k % 4 on the whole-frame paths).  Who read slot k % 4 last — gray image k-4:
        //  * equaliser on: CLAHE(k-4), nobody else (the equalised image is what detector, pyramid and KLT see);
        //  * equaliser off: detector(k-4) incl. cornerSubPix on its image stream, pyramid(k-4) (which copies it into level 0) on the side stream.
        // Run-ahead mode (single and batch handles, device polls or RVIO_PARANOID's stream events alike): book-keeping(k-4) followed pyramid(k-4) /
        // KLT(k-4) on the side stream and its refill half waited for the corners of detector(k-4); book-keeping(k-3) followed it there, and the wait
        // above puts this launch behind book-keeping(k-3) — the wait that protects equalised image k % 4 and corner list k % 3 covers the gray slot
        // too (with two image chains, or one at long windows, CLAHE(k-4) also sits earlier on this very stream).
        // Every other mode — RVIO_NO_RUNAHEAD, a caller-side corner list, the per-stage calls — has ONE image stream for every frame: CLAHE /
        // detector of earlier images are earlier on it, and a pyramid that ran on the side stream was joined back into it in front of that
        // image's book-keeping (post_klt_dev).  No wait of its own anywhere.
        h->gray_slot = (h->gray_slot + 1) % 4;
        uint8_t* g = h->d_gray[h->gray_slot];
        launch_gray(h, f, d_img, stride, src_bs, g, is);
        d_img = g; stride = d.W; src_bs = (size_t)d.W * d.H;
    }
    if (f.clahe_lut != LPCL_NONE) {   // clahe->apply(im, im), Tracker.cc:198-202
        // The equalised image of frame k doubles as level 0 of frame k's pyramid (no copy), so it lives until the KLT of frame k+1 has
        // matched against it: four buffers in rotation (like the pyramids, and three corner lists).  Slot k % 4 was last read by KLT(k-3)
        // (as the previous image) and by the detector / pyramid of frame k-4; in run-ahead mode CLAHE(k) waits for book-keeping(k-3), which
        // followed KLT(k-3) on the side stream and was the last reader of corner list k % 3.  (With three / three / two buffers the wait
        // was for book-keeping(k-2): an image chain is ~190 us long, so it started late enough to hold book-keeping(k) up.)
        h->eq_slot = (h->eq_slot + 1) % 4;
        uint8_t* eq = h->d_eq2[h->eq_slot];
        uint8_t* lut = h->d_lut2[f.lut_set];
        const dim3 lg = lp_grid(f.clahe_lut_l), lb = lp_block(f.clahe_lut_l), ig = lp_grid(f.clahe_interp_l), ib = lp_block(f.clahe_interp_l);
        switch (f.clahe_lut) {
        case LPCL_NONE: break;
        case LPCL_COL16_256X8:
            hipLaunchKernelGGL((clahe_lut_kernel2<256, 8>), lg, lb, 0, is, d_img, d.W, d.H, stride, h->cl_tx, h->cl_tw, h->cl_th, h->cl_clip, h->cl_scale, lut, src_bs, bs, (int)h->frame_no);
            break;
        case LPCL_COL16_1024:
            hipLaunchKernelGGL(clahe_lut_kernel2<1024>, lg, lb, 0, is, d_img, d.W, d.H, stride, h->cl_tx, h->cl_tw, h->cl_th, h->cl_clip, h->cl_scale, lut, src_bs, bs, (int)h->frame_no);
            break;
        case LPCL_WAVE32:
            hipLaunchKernelGGL(clahe_lut_kernel, lg, lb, 0, is, d_img, d.W, d.H, stride, h->cl_tx, h->cl_tw, h->cl_th, h->cl_clip, h->cl_scale, lut, src_bs, bs, (int)h->frame_no);
            break;
        }
        switch (f.clahe_interp) {
        case LPCI_NONE: break;
        case LPCI_PX4:
            hipLaunchKernelGGL(clahe_interp_kernel4, ig, ib, 0, is, d_img, d.W, d.H, stride, h->cl_tx, h->cl_ty, 1.0f / (float)h->cl_tw, 1.0f / (float)h->cl_th, lut, eq, src_bs, bs);
            break;
        case LPCI_PX1:
            hipLaunchKernelGGL(clahe_interp_kernel, ig, ib, 0, is, d_img, d.W, d.H, stride, h->cl_tx, h->cl_ty, 1.0f / (float)h->cl_tw, 1.0f / (float)h->cl_th, lut, eq, src_bs, bs);
            break;
        }
        d_img = eq; stride = d.W; src_bs = bs;
        if (f.pyr_on_image) {   // the side stream (KLT) waits for the pyramid of the equalised image; the detector follows on the image stream itself
            launch_pyramid(is);
            if (f.klt_polls_pyramid) {   // the counter is bumped by the detector's first launch on this queue (detect_dev), right behind the pyramid
                h->stage_tgt.pyr[f.ic]++;
                klt->counter = &h->stage_sync->pyr[f.ic]; klt->target = h->stage_tgt.pyr[f.ic];
            } else {
                HIPCHK(h, hipEventRecord(h->evC[f.ic], is));
                HIPCHK(h, hipStreamWaitEvent(h->stream_d, h->evC[f.ic], 0));
            }
        }
    }
    if (f.use_det) {   // FeatureDetector::DetectWithSubPix on the image the tracker sees (Tracker.cc:207,350)
        if (f.fork_side) {   // fork: pyramid / KLT / RANSAC go to the side stream (the image is complete on the image stream here), the detector stays
            HIPCHK(h, hipEventRecord(h->evD0, is));
            HIPCHK(h, hipStreamWaitEvent(h->stream_d, h->evD0, 0));
        }
        const int rc = detect_dev(h, f, d_img, stride, src_bs);
        if (rc != RVIO_OK) return rc;
        switch (f.corners) {   // corners of frame k ready: the refill half of book-keeping on the side stream waits for it
        case LPA_NONE: break;
        case LPA_SIGNAL: hipLaunchKernelGGL(stage_signal_kernel, dim3(1), dim3(64), 0, is, &h->stage_sync->corners[f.ic]); h->stage_tgt.corners[f.ic]++; break;
        case LPA_EVENT: HIPCHK(h, hipEventRecord(h->evD1, is)); break;
        }
    }
    if (!f.pyr_on_image) launch_pyramid(stream_of(h, f.pyr, f.ic));
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}

// everything after Tracker.cc:246; status/tracked already on the device
static int post_klt_dev(rvio_hip* h, const FrontForms& f, const rvio_imu* d_imu, int m, const float* d_cand, int n_cand, const BookWait& bw, BookOut* out) {
    const size_t bs = h->slab_bytes;
    const hipStream_t base = stream_of(h, f.base, f.ic), side = stream_of(h, f.side, f.ic), tail = stream_of(h, f.book, f.ic);
    // (standstill detection, rvio_hip_standstill*: the detector reads what this book-keeping rewrites.  It ran on the stream of the LAST book-keeping;
    // if this one runs elsewhere — the call mode changed — its stream waits for the detector.  A handle without the feature never gets here)
    if (h->ss_last && h->ss_last != tail) HIPCHK(h, hipStreamWaitEvent(tail, h->evSSb, 0));
    h->ss_last = nullptr;
    h->book_stream = tail;
    const LpLaunch &lr = f.ransac_l, &la = f.book_a_l, &lb = f.book_b_l;
    const float* xy = h->det_xy2[f.dslot];      // the detector's corner list replaces the caller's
    const int* nout = h->det_nout + f.dslot;
    const unsigned long long* const no_counter = nullptr;
    *out = BookOut{};
    switch (f.book_form) {
    case LPB_PLAIN:
        hipLaunchKernelGGL(ransac_kernel, lp_grid(lr), lp_block(lr), lr.lds, side, h->dc, h->t.n_pts, h->t.tracked, h->t.un1, h->t.un2, h->t.status, d_imu, m, h->rng, h->d_info, bs, h->imu_bs, (const CamCal*)h->cal);
        hipLaunchKernelGGL(bookkeep_a_kernel, lp_grid(la), lp_block(la), 0, base, h->dc, h->t, (size_t)0, no_counter, 0ull, h->meta, (unsigned long long*)nullptr);
        hipLaunchKernelGGL(bookkeep_b_kernel, lp_grid(lb), lp_block(lb), lb.lds, base, h->dc, h->t, d_cand, n_cand, (const int*)nullptr, (size_t)0, no_counter, 0ull, h->meta, (const CamCal*)h->cal);
        break;
    case LPB_JOIN:   // join the side stream (long finished when the detector is)
        hipLaunchKernelGGL(ransac_kernel, lp_grid(lr), lp_block(lr), lr.lds, side, h->dc, h->t.n_pts, h->t.tracked, h->t.un1, h->t.un2, h->t.status, d_imu, m, h->rng, h->d_info, bs, h->imu_bs, (const CamCal*)h->cal);
        HIPCHK(h, hipEventRecord(h->evD1, side));
        HIPCHK(h, hipStreamWaitEvent(base, h->evD1, 0));
        hipLaunchKernelGGL(bookkeep_a_kernel, lp_grid(la), lp_block(la), 0, tail, h->dc, h->t, bs, no_counter, 0ull, h->meta, (unsigned long long*)nullptr);
        hipLaunchKernelGGL(bookkeep_b_kernel, lp_grid(lb), lp_block(lb), lb.lds, tail, h->dc, h->t, xy, 0, nout, bs, no_counter, 0ull, h->meta, (const CamCal*)h->cal);
        break;
    case LPB_FUSED:
    case LPB_PAIR: {   // book-keeping on the side stream, behind RANSAC: the hand-over half once the filter that read the table last has let go of it, the refill half once the corners are there
        if (bw.evt) HIPCHK(h, hipStreamWaitEvent(side, bw.evt, 0));
        const unsigned long long* done = bw.dev ? &h->stage_sync->aug : nullptr;
        const unsigned long long done_target = bw.dev ? bw.target : 0;
        unsigned long long* hand = nullptr;
        if (f.dev_sync) { hand = &h->stage_sync->handover; h->stage_tgt.handover++; }
        if (f.book_form == LPB_FUSED) {
            out->gate = true; out->gate_target = h->stage_tgt.handover;
            hipLaunchKernelGGL(ransac_book_kernel, lp_grid(lr), lp_block(lr), lr.lds, tail, h->dc, h->t, d_imu, m, h->rng, bs, h->imu_bs,
                               done, done_target, h->meta, hand, xy, nout, &h->stage_sync->corners[f.ic], h->stage_tgt.corners[f.ic], (const CamCal*)h->cal);
            break;
        }
        hipLaunchKernelGGL(ransac_book_a_kernel, lp_grid(lr), lp_block(lr), lr.lds, tail, h->dc, h->t, d_imu, m, h->rng, bs, h->imu_bs, done, done_target, h->meta, hand, (const CamCal*)h->cal);
        // the Updater's input is complete: the filter of this frame waits for THIS — the gate kernel on the filter stream polls the
        // counter the launch above bumps, and the refill half below polls the detector's; or two stream-level events
        const unsigned long long* corners = nullptr; unsigned long long corners_target = 0;
        if (f.dev_sync) { out->gate = true; out->gate_target = h->stage_tgt.handover; corners = &h->stage_sync->corners[f.ic]; corners_target = h->stage_tgt.corners[f.ic]; }
        else {
            HIPCHK(h, hipEventRecord(h->evH[h->frame_no & 3], tail));
            out->handover_evt = true;
            HIPCHK(h, hipStreamWaitEvent(side, h->evD1, 0));
        }
        hipLaunchKernelGGL(bookkeep_b_kernel, lp_grid(lb), lp_block(lb), lb.lds, tail, h->dc, h->t, xy, 0, nout, bs, corners, corners_target, h->meta, (const CamCal*)h->cal);
        break;
    }
    }
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}

static int track_dev_impl(rvio_hip* h, const FrontForms& f, const uint8_t* d_img, int stride, const rvio_imu* d_imu, int m, const float* d_cand, int n_cand,
                          const BookWait& bw, BookOut* out) {
    HIPCHK(h, hipSetDevice(h->device));
    if (h->piped && !f.piped) SYNC_FRONT(h);
    int rc;
    if (f.use_det && (rc = detector_init(h)) != RVIO_OK) return rc;
    const int nb = (h->pyr_cur + 1) % 4;   // pyramid of the new image; pyr_cur holds mLastImage's (slot nb was last read by KLT(k-3))
    KltWait kw;
    rc = build_pyramid_dev(h, f, d_img, stride, nb, &kw);
    if (rc != RVIO_OK) return rc;
    const hipStream_t side = stream_of(h, f.side, f.ic);
    switch (f.klt) {
    case LPKL_K16:
        hipLaunchKernelGGL(klt_kernel16, lp_grid(f.klt_l), lp_block(f.klt_l), 0, side, h->pyr[h->pyr_cur], h->pyr[nb], h->dc.levels, h->t.n_pts, h->t.feats, h->t.tracked, h->t.status, h->slab_bytes);
        break;
    case LPKL_K3:
        hipLaunchKernelGGL(klt_kernel3, lp_grid(f.klt_l), lp_block(f.klt_l), 0, side, h->pyr[h->pyr_cur], h->pyr[nb], h->dc.levels, h->t.n_pts, h->t.feats, h->t.tracked, h->t.status, h->slab_bytes,
                           kw.counter, kw.target, h->meta);
        break;
    }
    rc = post_klt_dev(h, f, d_imu, m, d_cand, std::min(n_cand, h->dc.F), bw, out);
    h->pyr_cur = nb;   // im.copyTo(mLastImage), Tracker.cc:395
    h->last.dslot = f.dslot;
    if (f.use_det) h->last.det_set = f.det_set;
    if (f.gray != LPGR_NONE) { h->last.gray_src = d_img; h->last.gray_stride = stride; h->last.gray_bs = h->img_bs; }
    return rc;
}
int rvio_hip_track_dev(rvio_hip* h, const uint8_t* d_img, int stride, const rvio_imu* d_imu, int m, const float* d_cand, int n_cand) {
    if (!h || !d_img || m < 0 || n_cand < 0 || check_image(h, d_img, stride, 0) != RVIO_OK) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    if (!d_cand) refresh_first_cleared(h);
    const FrontForms f = call_forms(h, false, d_cand != nullptr, d_img, stride, h->img_bs);   // a per-stage call: everything on the filter stream
    BookOut bo;
    return track_dev_impl(h, f, d_img, stride, d_imu, m, d_cand, n_cand, BookWait{}, &bo);
}

int rvio_hip_track(rvio_hip* h, const uint8_t* img, int stride, const rvio_imu* imu, int m, const float* cand_xy, int n_cand) {
    if (!h || !img || (!imu && m > 0) || m < 0 || n_cand < 0 || check_image(h, nullptr, stride, 0) != RVIO_OK) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    { const int rcg = ensure_imu_capacity(h, m); if (rcg != RVIO_OK) return rcg; }
    const int nc = std::min(n_cand, h->dc.F);
    const int rowb = h->dc.W * h->pix_ch;   // bytes of an image row (interleaved pixels with a colour format)
    HIPCHK(h, hipMemcpy2DAsync(h->d_img, rowb, img, stride, rowb, h->dc.H, hipMemcpyHostToDevice, h->stream));
    if (m > 0) HIPCHK(h, hipMemcpyAsync(h->d_imu, imu, sizeof(rvio_imu) * m, hipMemcpyHostToDevice, h->stream));
    if (nc > 0 && cand_xy) HIPCHK(h, hipMemcpyAsync(h->d_cand, cand_xy, sizeof(float) * 2 * nc, hipMemcpyHostToDevice, h->stream));
    return rvio_hip_track_dev(h, h->d_img, rowb, h->d_imu, m, cand_xy ? h->d_cand : nullptr, cand_xy ? nc : 0);
}

// direct-track mode: the caller supplies the KLT result
int rvio_hip_track_points(rvio_hip* h, const float* tracked_xy, const unsigned char* status, int n_pts,
                          const rvio_imu* imu, int m, const float* cand_xy, int n_cand) {
    if (!h || (!imu && m > 0) || m < 0 || n_cand < 0 || n_pts < 0 || n_pts > h->dc.F) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    { const int rcg = ensure_imu_capacity(h, m); if (rcg != RVIO_OK) return rcg; }
    const int nc = std::min(n_cand, h->dc.F);
    if (n_pts > 0) {
        HIPCHK(h, hipMemcpyAsync(h->d_in_xy, tracked_xy, sizeof(float) * 2 * n_pts, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_in_st, status, n_pts, hipMemcpyHostToDevice, h->stream));
    }
    if (m > 0) HIPCHK(h, hipMemcpyAsync(h->d_imu, imu, sizeof(rvio_imu) * m, hipMemcpyHostToDevice, h->stream));
    if (nc > 0) HIPCHK(h, hipMemcpyAsync(h->d_cand, cand_xy, sizeof(float) * 2 * nc, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(load_points_kernel, dim3(8), dim3(256), 0, h->stream, h->t.n_pts, h->d_in_xy, h->d_in_st, h->t.tracked, h->t.status);   // (single instance only)
    const FrontForms f = call_forms(h, false, true, nullptr, 0, 0);   // no image in this mode: the caller's corner list, everything on the filter stream
    BookOut bo;
    return post_klt_dev(h, f, h->d_imu, m, h->d_cand, nc, BookWait{}, &bo);
}

int rvio_hip_get_tracks(rvio_hip* h, int32_t* n_feat, unsigned char* types, int32_t* len, float* meas) {
    if (!h) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    SYNC_FRONT(h);   // image / side / tracker streams first
    const DevCfg& d = h->dc;
    int nf = 0;
    HIPCHK(h, hipMemcpyAsync(&nf, h->t.n_feat, sizeof nf, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n_feat) *n_feat = nf;
    if (nf > 0) {
        if (types) HIPCHK(h, hipMemcpyAsync(types, h->t.types, nf, hipMemcpyDeviceToHost, h->stream));
        if (len) HIPCHK(h, hipMemcpyAsync(len, h->t.len, sizeof(int) * nf, hipMemcpyDeviceToHost, h->stream));
        if (meas) HIPCHK(h, hipMemcpyAsync(meas, h->t.meas, sizeof(float) * 2 * d.max_len * nf, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}

// mvFeatsToTrack and the length of each feature's tracking history, of one instance
int rvio_hip_get_tracker_points_at(rvio_hip* h, int instance, int32_t* n, float* xy, int32_t* hist_len) {
    if (!h || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    if (!h->front_end) { h->err = "this batch handle was created without its front end"; return RVIO_ERR_UNSUPPORTED; }
    HIPCHK(h, hipSetDevice(h->device));
    SYNC_FRONT(h);   // image / side / tracker streams first
    const DevCfg& d = h->dc;
    const size_t o = (size_t)instance * h->slab_bytes;
    int np = 0;
    HIPCHK(h, hipMemcpyAsync(&np, (char*)h->t.n_pts + o, sizeof np, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n) *n = np;
    if (np > 0) {
        if (xy) HIPCHK(h, hipMemcpyAsync(xy, (char*)h->t.feats + o, sizeof(float) * 2 * np, hipMemcpyDeviceToHost, h->stream));
        if (hist_len) {
            std::vector<int> slot(np), hl(d.F);
            HIPCHK(h, hipMemcpyAsync(slot.data(), (char*)h->t.slot + o, sizeof(int) * np, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipMemcpyAsync(hl.data(), (char*)h->t.hist_len + o, sizeof(int) * d.F, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            for (int i = 0; i < np; ++i) hist_len[i] = hl[slot[i]];
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}
int rvio_hip_get_tracker_points(rvio_hip* h, int32_t* n, float* xy, int32_t* hist_len) {
    if (!h) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    return rvio_hip_get_tracker_points_at(h, 0, n, xy, hist_len);
}

// ------------------------------------------------------------------ whole frame (System.cc:253-367)
// Pieces for callers that sequence the frame themselves (staged timing, sharded updater):
// frame_plan advances nImageCountAfterInit and reports MonoVIO's two data-independent branches.
int rvio_hip_frame_plan(rvio_hip* h, int* do_update, int* do_augment) {
    if (!h) return RVIO_ERR_INVALID;
    h->img_count++;
    if (do_update) *do_update = (h->n_clones_host > h->cfg.min_track_len - 1) ? 1 : 0;   // System.cc:266
    if (do_augment) *do_augment = (h->img_count > 1) ? 1 : 0;                            // System.cc:280
    return RVIO_OK;
}
int rvio_hip_propagate_dev(rvio_hip* h, const rvio_imu* d_imu, int m) {
    if (!h || (!d_imu && m > 0) || m < 0) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    return propagate_dev(h, d_imu, m);
}

// `stream` goes on once the filter of the last frame with parity b has finished (see fin_mode)
static int wait_filter_done(rvio_hip* h, int b, hipStream_t stream) {
    if (h->fin_mode[b] == 0) HIPCHK(h, hipStreamWaitEvent(stream, h->evF[b], 0));
    else HIPCHK(h, hipStreamSynchronize(h->stream));   // (a call that left run-ahead mode: rare, the host waits)
    return RVIO_OK;
}
static int frame_tail_dev(rvio_hip* h, const rvio_imu* d_imu, int m, bool propagated = false) {
    h->img_count++;
    int rc = propagated ? RVIO_OK : propagate_dev(h, d_imu, m);
    if (rc != RVIO_OK) return rc;
    if (h->n_clones_host > h->cfg.min_track_len - 1) {   // System.cc:266
        rc = rvio_hip_update_tracked(h);
        if (rc != RVIO_OK) return rc;
    }
    return augment_compose_dev(h, h->img_count > 1);      // System.cc:280
}
// The body of System::MonoVIO after Tracker::track (System.cc:263-365) on device-resident hand-over tables, for every instance
// of the handle in ONE launch per stage: d_n_feat[B], d_types[B][Fu], d_len[B][Fu], d_meas[B][Fu][max_track_len][2] (the layout
// of rvio_tracks with max_len = max_track_len), d_imu[B][imu_stride] (imu_stride = 0: one IMU batch shared by all instances).
int rvio_hip_frame_tracks_dev(rvio_hip* h, const rvio_imu* d_imu, int imu_stride, int m, const int32_t* d_n_feat, const unsigned char* d_types,
                              const int32_t* d_len, const float* d_meas) {
    if (!h || (!d_imu && m > 0) || m < 0 || imu_stride < 0 || (imu_stride > 0 && imu_stride < m)) return RVIO_ERR_INVALID;
    if (!d_n_feat || !d_types || !d_len || !d_meas) return RVIO_ERR_INVALID;
    if (h->piped || h->in_frame) { h->err = "rvio_hip_frame_tracks_dev on a handle that runs the pipelined image path"; return RVIO_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    const DevCfg& d = h->dc;
    h->img_count++;
    const bool upd = h->n_clones_host > h->cfg.min_track_len - 1;   // System.cc:266
    // A filter-only batch: PreIntegrator::propagate (one latency-bound workgroup per instance, two per CU) runs on the handle's second stream
    // BESIDE the per-feature stage of the update — U1-U5 and the share reduction read only the clone states and P[24:,24:], which propagation does
    // not touch (the reason feat_prop_kernel may fuse them for one stream) — and joins in front of the solve, which needs the propagated rows.
    const bool overlap = upd && h->batch > 1 && !h->front_end;
    int rc;
    if (overlap) {
        HIPCHK(h, hipEventRecord(h->evD0, h->stream));
        HIPCHK(h, hipStreamWaitEvent(h->stream_t, h->evD0, 0));
        rc = propagate_dev(h, d_imu, m, (size_t)imu_stride * sizeof(rvio_imu), h->stream_t);
        HIPCHK(h, hipEventRecord(h->evD1, h->stream_t));
    } else rc = propagate_dev(h, d_imu, m, (size_t)imu_stride * sizeof(rvio_imu));
    if (rc != RVIO_OK) return rc;
    if (upd) {
        const TrackerDev t0 = h->t;
        const BatchIn b0 = h->bin;
        h->t.n_feat = const_cast<int*>(d_n_feat); h->t.types = const_cast<unsigned char*>(d_types);
        h->t.len = const_cast<int*>(d_len); h->t.meas = const_cast<float*>(d_meas);
        h->bin = {0, sizeof(int32_t), (size_t)d.Fu, sizeof(int32_t) * (size_t)d.Fu, sizeof(float) * 2 * (size_t)d.Fu * d.max_len};
        rc = update_local_dev(h, 0, 1, true);
        if (overlap) HIPCHK(h, hipStreamWaitEvent(h->stream, h->evD1, 0));
        if (rc == RVIO_OK) rc = update_global_dev(h, h->block, 1, true);
        h->t = t0; h->bin = b0;
        if (rc != RVIO_OK) return rc;
    }
    return augment_compose_dev(h, h->img_count > 1);      // System.cc:280
}

// Pipelined: the tracker (pyramid, KLT, RANSAC, book-keeping) never reads the filter state, so frame k's front end runs
// on its own stream while frame k-1's propagate/update/augment still occupy the filter stream.  The Tracker -> Updater
// hand-over is double-buffered; two events per buffer order (a) update(k) after track(k), (b) track(k+2) after update(k).
// PreIntegrator::propagate needs nothing from the tracker either: it is enqueued first and runs beside the front end.
// the forms of a whole-frame call (the entry points compute them: rvio_hip_frame needs the mode ahead of its staging copies)
static FrontForms frame_forms(rvio_hip* h, const uint8_t* d_img, int stride, const float* d_cand) {
    if (!d_cand) refresh_first_cleared(h);
    return call_forms(h, true, d_cand != nullptr, d_img, stride, h->img_bs);
}
static int frame_dev_impl(rvio_hip* h, const FrontForms& f, const uint8_t* d_img, int stride, const rvio_imu* d_imu, int m, const float* d_cand, int n_cand, bool staged,
                          bool begin_only = false, bool defer_propagate = false) {   // defer_propagate: the caller runs update_local_dev itself right behind (the sharded frame)
    if (h->in_frame) { h->err = "rvio_hip_frame_begin_dev without rvio_hip_frame_end"; return RVIO_ERR_INVALID; }
    const int b = (int)(h->frame_no & 1);                   // parity: the staging of rvio_hip_frame
    const int hb = (int)(h->frame_no % rvio_hip::kHand);    // hand-over table of this frame
    h->t.n_feat = h->tout[hb].n_feat; h->t.types = h->tout[hb].types; h->t.len = h->tout[hb].len; h->t.meas = h->tout[hb].meas;
    BookWait bw;   // run-ahead mode: book-keeping runs on the side stream, and what it has to wait for goes there with it
    if (h->frame_no >= rvio_hip::kHand) {   // the filter of frame k - kHand has consumed this hand-over buffer: only the stream that runs book-keeping has to know.
        // (In run-ahead mode the image chains — CLAHE, detector — never touch the hand-over: making them wait here tied image(k) to
        // filter(k-2) and with it the frame period to image chain + filter chain over two frames.)
        // Run-ahead: of the side stream's chain (pyramid, KLT, RANSAC, book-keeping) only book-keeping writes the hand-over, so the wait
        // goes right in front of it (post_klt_dev) — at the head of the frame it tied KLT(k) to filter(k-2) and made
        // [side chain + filter chain] the period of two frames.
        if (!f.runahead) { int rcw = wait_filter_done(h, hb, h->stream_t); if (rcw == RVIO_OK) rcw = wait_filter_done(h, hb, h->stream_d); if (rcw != RVIO_OK) return rcw; }
        else if (h->fin_mode[hb] == 0) bw.evt = h->evF[hb];
        else { bw.dev = true; bw.target = h->fin_target[hb]; }
    } else if (!h->piped) HIPCHK(h, hipStreamSynchronize(h->stream));   // first pipelined frame: everything enqueued so far is done
    h->piped = true;
    if (m < 0) return RVIO_ERR_INVALID;
#ifdef RVIO_DBG_CLOCKS
    static const bool dbg_host = getenv("RVIO_DBG_HOST") != nullptr;   // host-side enqueue times on stderr (selects nothing)
#else
    constexpr bool dbg_host = false;
#endif
    static double acc[5] = {0, 0, 0, 0, 0}; static long nacc = 0;
    auto now = []() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = dbg_host ? now() : 0;
    if (staged) {   // the IMU batch was copied on the tracker stream (run-ahead: the side stream): propagate (filter stream) and RANSAC need it
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->evIn[b], 0));
        HIPCHK(h, hipStreamWaitEvent(h->stream_d, h->evIn[b], 0));
    }
    // propagate: with an update in this frame (and nobody sequencing the update from outside) it rides in the per-feature launch,
    // otherwise it goes to the filter stream right behind augment/compose(k-1)
    const bool fuse = h->plan.fuse_ok && (!begin_only || defer_propagate) && h->n_clones_host > h->cfg.min_track_len - 1;
    int rc = RVIO_OK;
    h->fuse_m = -1;
    if (!fuse) rc = propagate_dev(h, d_imu, m, h->imu_bs, nullptr, h->img_count + 1);   // (this frame's count: frame_tail_dev / rvio_hip_frame_plan advance it behind this call)
    if (rc != RVIO_OK) return rc;
    const double t1 = dbg_host ? now() : 0;
    BookOut bo;
    rc = track_dev_impl(h, f, d_img, stride, d_imu, m, d_cand, n_cand, bw, &bo);
    if (rc != RVIO_OK) return rc;
    const double t2 = dbg_host ? now() : 0;
    HIPCHK(h, hipEventRecord(h->evT[h->frame_no & 3], stream_of(h, f.book, f.ic)));      // behind book-keeping, on the stream that ran it
    // the filter needs the hand-over, not the refill: in run-ahead mode it waits for the first half of book-keeping only
    if (bo.gate) hipLaunchKernelGGL(stage_gate_kernel, dim3(1), dim3(64), 0, h->stream, &h->stage_sync->handover, bo.gate_target, h->meta, h->t.n_feat, (int)h->frame_no);
    else HIPCHK(h, hipStreamWaitEvent(h->stream, bo.handover_evt ? h->evH[h->frame_no & 3] : h->evT[h->frame_no & 3], 0));
    const double t3 = dbg_host ? now() : 0;
    if (begin_only) {   // the caller sequences update / augment itself, then rvio_hip_frame_end
        h->in_frame = true;
        if (fuse) { h->fuse_imu = d_imu; h->fuse_m = m; }   // (the sharded frame: consumed by its update_local_dev, same condition)
        return RVIO_OK;
    }
    if (fuse) { h->fuse_imu = d_imu; h->fuse_m = m; }   // consumed by the per-feature launch of this frame's update (same condition: it runs)
    if (fuse) { h->time_imu = d_imu; h->time_m = m; h->time_imu_bs = 0; }
    rc = frame_tail_dev(h, d_imu, m, /*propagated=*/true);
    h->fuse_m = -1;
    const double t4 = dbg_host ? now() : 0;
    // the filter of this frame is finished when ... single instance in run-ahead mode: its last kernel has bumped the device-side counter
    // (book-keeping of frame k+2 polls it); otherwise an event behind it
    if (f.filter_done_by_counter) { h->fin_mode[hb] = 1; h->fin_target[hb] = h->stage_tgt.aug; }
    else { HIPCHK(h, hipEventRecord(h->evF[hb], h->stream)); h->fin_mode[hb] = 0; }
    if (dbg_host) {
        const double t5 = now();
        acc[0] += t1 - t0; acc[1] += t2 - t1; acc[2] += t3 - t2; acc[3] += t4 - t3; acc[4] += t5 - t4;
        if (++nacc % 100 == 0) { std::fprintf(stderr, "host us/frame: propagate %.1f track %.1f evT %.1f tail %.1f evF %.1f\n", acc[0] / 100, acc[1] / 100, acc[2] / 100, acc[3] / 100, acc[4] / 100); for (double& a : acc) a = 0; }
    }
    h->frame_no++;
    if (rc == RVIO_OK && (paranoid_bits() & PAR_DRAIN)) rc = drain_all(h);
    return rc;
}
int rvio_hip_frame_dev(rvio_hip* h, const uint8_t* d_img, int stride, const rvio_imu* d_imu, int m, const float* d_cand, int n_cand) {
    if (!h || !d_img || check_image(h, d_img, stride, 0) != RVIO_OK) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    return frame_dev_impl(h, frame_forms(h, d_img, stride, d_cand), d_img, stride, d_imu, m, d_cand, n_cand, false);
}
// One camera frame of EVERY instance of a batch handle created with its front end: d_imgs[B] (instance stride img_stride bytes,
// row stride `stride`), d_imu[B][imu_stride] (0: shared).  Same pipelined body as rvio_hip_frame_dev, every launch with gridDim.z = B;
// corners always come from the device detector.
int rvio_hip_frame_batch_dev(rvio_hip* h, const uint8_t* d_imgs, int stride, size_t img_stride, const rvio_imu* d_imu, int imu_stride, int m) {
    if (!h || !d_imgs || (!d_imu && m > 0) || imu_stride < 0 || (imu_stride > 0 && imu_stride < m) || check_image(h, d_imgs, stride, h->batch > 1 ? img_stride : 0) != RVIO_OK) return RVIO_ERR_INVALID;
    if (!h->front_end) { h->err = "this batch handle was created without its front end"; return RVIO_ERR_UNSUPPORTED; }
    if (h->batch > 1 && img_stride < (size_t)stride * h->dc.H) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    h->img_bs = img_stride; h->imu_bs = (size_t)imu_stride * sizeof(rvio_imu);
    const int rc = frame_dev_impl(h, frame_forms(h, d_imgs, stride, nullptr), d_imgs, stride, d_imu, m, nullptr, 0, false);
    h->img_bs = 0; h->imu_bs = 0;
    return rc;
}
// The pipelined frame split open for callers that sequence the update themselves (the feature-sharded updater):
//   frame_begin_dev   propagate on the filter stream, the front end on its streams, filter stream ordered after the front end
//   ... rvio_hip_frame_plan, rvio_hip_update_local / collective / rvio_hip_update_global (or update_tracked), rvio_hip_augment_compose,
//       all on the filter stream (rvio_hip_stream) ...
//   frame_end         closes the frame (hand-over buffer released for frame k+2)
int rvio_hip_frame_begin_dev(rvio_hip* h, const uint8_t* d_img, int stride, const rvio_imu* d_imu, int m, const float* d_cand, int n_cand) {
    if (!h || !d_img || check_image(h, d_img, stride, 0) != RVIO_OK) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    return frame_dev_impl(h, frame_forms(h, d_img, stride, d_cand), d_img, stride, d_imu, m, d_cand, n_cand, false, /*begin_only=*/true);
}
int rvio_hip_frame_end(rvio_hip* h) {
    if (!h || !h->in_frame) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventRecord(h->evF[h->frame_no % rvio_hip::kHand], h->stream));
    h->fin_mode[h->frame_no % rvio_hip::kHand] = 0;
    h->frame_no++;
    h->in_frame = false;
    if (paranoid_bits() & PAR_DRAIN) return drain_all(h);
    return RVIO_OK;
}
// RCCL's ncclAllGather, resolved at run time from the RCCL instance the process has ALREADY loaded (the communicator the caller hands over
// belongs to it: torch ships its own librccl.so) and only then from the system's.  No link-time dependency: a single-GPU user never loads RCCL.
typedef int (*nccl_allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
static nccl_allgather_fn resolve_allgather(std::string* why) {
    static nccl_allgather_fn fn = nullptr;
    if (fn) return fn;
    void* lib = nullptr;
    for (const char* name : {"librccl.so", "librccl.so.1"}) if ((lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD))) break;
    if (!lib) {   // torch's copy is loaded by path, not by soname lookup: look for a loaded object whose name ends in librccl.so*
        fn = (nccl_allgather_fn)dlsym(RTLD_DEFAULT, "ncclAllGather");
        if (fn) return fn;
    }
    if (!lib) for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) if ((lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (lib) fn = (nccl_allgather_fn)dlsym(lib, "ncclAllGather");
    if (!fn && why) *why = "ncclAllGather not found (no librccl.so loaded or loadable)";
    return fn;
}
// One pipelined frame with the feature-sharded updater behind ONE call: the front end and propagate replicated, U1-U5 + the
// share reduction on the features f % world == rank, ONE ncclAllGather of the [S2 | S1] blocks enqueued on the filter stream between the two
// kernels it separates (plain stream order: no helper stream, no event, no host synchronisation), the replicated global stage, augmentation /
// composition.  comm: the caller's ncclComm_t; NULL only with world == 1 (the collective is skipped).  allgather: NULL = resolve RCCL's
// ncclAllGather from the loaded process image; a caller may hand in the entry point itself (same signature).
int rvio_hip_frame_sharded_dev(rvio_hip* h, const uint8_t* d_img, int stride, const rvio_imu* d_imu, int m, const float* d_cand, int n_cand,
                               int rank, int world, void* comm, void* allgather) {
    if (!h || !d_img || world < 1 || rank < 0 || rank >= world || (!comm && world > 1) || check_image(h, d_img, stride, 0) != RVIO_OK) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    if (comm) h->extra_queues = true;   // the collective brings queues of its own: more than the four this handle's chains own (see the pyramid poll, build_pyramid_dev)
    const size_t nblk_max = (size_t)shard_payload_doubles(6 * h->dc.nmax, h->dc.max_len);    // the full window's payload: what the receive buffer is sized for
    nccl_allgather_fn ag = (nccl_allgather_fn)allgather;
    if (comm && !ag && !(ag = resolve_allgather(&h->err))) return RVIO_ERR_UNSUPPORTED;
    if (comm && h->gathered_world < world) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        // (a larger world: the old block stays, freed with the handle)
        RCCHK(own_dev(h, &h->gathered, sizeof(double) * nblk_max * (size_t)world));
        h->gathered_world = world;
    }
    int rc = frame_dev_impl(h, frame_forms(h, d_img, stride, d_cand), d_img, stride, d_imu, m, d_cand, n_cand, false, /*begin_only=*/true, /*defer_propagate=*/true);
    if (rc != RVIO_OK) return rc;
    h->img_count++;
    if (h->n_clones_host > h->cfg.min_track_len - 1) {   // System.cc:266
        rc = update_local_dev(h, rank, world, false);
        const double* blocks = h->block;
        if (rc == RVIO_OK && comm) {
            const size_t nblk = (size_t)shard_payload_doubles(6 * h->n_clones_host, h->dc.max_len);     // (grows with the window: 8 + 256 doubles per carried tile)
            const int nrc = ag(h->block, h->gathered, nblk, /*ncclFloat64*/ 8, comm, h->stream);
            if (nrc != 0) { h->err = "ncclAllGather failed (ncclResult_t " + std::to_string(nrc) + ")"; rc = RVIO_ERR_NO_DEVICE; }
            blocks = h->gathered;
        }
        if (rc == RVIO_OK) rc = update_global_dev(h, blocks, world, false);
    }
    if (rc == RVIO_OK) rc = augment_compose_dev(h, h->img_count > 1);      // System.cc:280
    const int rce = rvio_hip_frame_end(h);
    return rc != RVIO_OK ? rc : rce;
}
// The same body fed from HOST buffers — what System::MonoVIO holds at System.cc:253 (a cv::Mat and the IMU list).
// The three H2D copies go to the tracker stream into staging buffers double-buffered by frame parity, so they overlap
// the previous frame's filter work like the tracker kernels do.
int rvio_hip_frame(rvio_hip* h, const uint8_t* img, int stride, const rvio_imu* imu, int m, const float* cand_xy, int n_cand) {
    if (!h || !img || (!imu && m > 0) || m < 0 || n_cand < 0 || check_image(h, nullptr, stride, 0) != RVIO_OK) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    { const int rcg = ensure_imu_capacity(h, m); if (rcg != RVIO_OK) return rcg; }
    const int nc = cand_xy ? std::min(n_cand, h->dc.F) : 0;   // cand_xy == NULL: device detector
    if (!h->hb_img[0])
        for (int k = 0; k < 2; ++k) {
            DALLOC(h, h->hb_img[k], h->img_cap);
            DALLOC(h, h->hb_imu[k], (size_t)h->imu_cap);
            if (k == 1) for (int q = 2; q <= rvio_hip::kHand; ++q) DALLOC(h, h->hb_imu[q], (size_t)h->imu_cap);
            DALLOC(h, h->hb_cand[k], (size_t)2 * h->dc.F);
            HIPCHK(h, hipStreamSynchronize(h->stream));   // DALLOC clears on the filter stream
        }
    const size_t rowb = (size_t)h->dc.W * h->pix_ch, npx = rowb * h->dc.H;   // bytes of a row / of the image as staged (interleaved pixels with a colour format: gray_kernel converts them on the device)
    if (!h->pin[0]) {
        h->pin_img = 0; h->pin_imu = (npx + 255) & ~(size_t)255;
        const size_t pin_cand = h->pin_imu + ((sizeof(rvio_imu) * (size_t)h->imu_cap + 255) & ~(size_t)255);
        h->pin_bytes = pin_cand + sizeof(float) * 2 * h->dc.F;
        for (int k = 0; k < rvio_hip::kPin; ++k) {
            int rc = own_pinned(h, &h->pin[k], h->pin_bytes);
            if (rc == RVIO_OK && !h->evPin[k]) rc = own_event(h, &h->evPin[k], kEvFlags);     // (the ring is laid out again after drop_pin_ring)
            if (rc == RVIO_OK && !h->evPin2[k]) rc = own_event(h, &h->evPin2[k], kEvFlags);
            if (rc != RVIO_OK) { drop_pin_ring(h); return rc; }   // (the next call starts over: pin[0] says whether the ring exists)
        }
    }
    const int b = (int)(h->frame_no & 1);
    const int ps = (int)(h->frame_no % rvio_hip::kPin);
    uint8_t* pp = h->pin[ps];
    const size_t pin_cand = h->pin_imu + ((sizeof(rvio_imu) * (size_t)h->imu_cap + 255) & ~(size_t)255);
    HIPCHK(h, hipEventSynchronize(h->evPin[ps]));   // the copies issued from this slot three frames ago are done (no-op before its first use)
    HIPCHK(h, hipEventSynchronize(h->evPin2[ps]));
    if ((size_t)stride == rowb) std::memcpy(pp, img, npx);   // (a continuous cv::Mat: one copy)
    else for (int y = 0; y < h->dc.H; ++y) std::memcpy(pp + (size_t)y * rowb, img + (size_t)y * stride, rowb);
    if (m > 0) std::memcpy(pp + h->pin_imu, imu, sizeof(rvio_imu) * m);
    if (nc > 0) std::memcpy(pp + pin_cand, cand_xy, sizeof(float) * 2 * nc);
    // the forms of this frame, ahead of the staging copies: which streams they go to depends on the mode
    const FrontForms f = frame_forms(h, h->hb_img[b], (int)rowb, cand_xy);
    const bool ra = f.runahead;
    int imu_slot = b;
    if (ra) {
        // run-ahead mode.  The IMU batch goes to the SIDE stream (RANSAC runs there; propagate on the filter stream waits for evIn): it
        // has to wait for the filter of frame k-2 (the last reader of hb_imu[b]), and that wait must not sit in front of an image chain.
        // kHand + 1 IMU slots in rotation: slot k % (kHand + 1) was last read by filter(k - kHand - 1) / RANSAC(k - kHand - 1), and this copy follows
        // book-keeping(k-1) on the side stream, which waited for filter(k - 1 - kHand) — no wait of its own (one here would again put a filter in front of KLT(k)).
        imu_slot = (int)(h->frame_no % (rvio_hip::kHand + 1));
        if (!h->last_ra) for (int i = 0; i < rvio_hip::kHand && i < h->frame_no; ++i) { const int rcw = wait_filter_done(h, i, h->stream_d); if (rcw != RVIO_OK) return rcw; }
        if (h->frame_no < 2 && !h->piped) HIPCHK(h, hipStreamSynchronize(h->stream));
        if (m > 0) HIPCHK(h, hipMemcpyAsync(h->hb_imu[imu_slot], pp + h->pin_imu, sizeof(rvio_imu) * m, hipMemcpyHostToDevice, h->stream_d));
        HIPCHK(h, hipEventRecord(h->evIn[b], h->stream_d));
        HIPCHK(h, hipEventRecord(h->evPin[ps], h->stream_d));
        // The image goes to the stream of this frame's image chain (tracker stream / fourth stream in rotation).  hb_img[b]
        // was last read by frame k-2: its CLAHE / detector (same stream, earlier) and — without the equaliser — its pyramid on the side
        // stream, which book-keeping(k-2) followed.
        // (A colour format: hb_img[b] holds the interleaved pixels and has ONE reader, gray_kernel(k-2), the first launch of that frame's image
        // chain — on this very stream, since k-2 and k share their image chain with one or two chains in flight; the wait below is then more than needed.)
        hipStream_t is = stream_of(h, f.image, f.ic);
        if (h->frame_no >= 2) HIPCHK(h, hipStreamWaitEvent(is, h->evT[(h->frame_no - 2) & 3], 0));
        HIPCHK(h, hipMemcpyAsync(h->hb_img[b], pp, npx, hipMemcpyHostToDevice, is));
        HIPCHK(h, hipEventRecord(h->evPin2[ps], is));
    } else {
        if (h->frame_no >= 2) { const int rcw = wait_filter_done(h, (int)((h->frame_no - 2) % rvio_hip::kHand), h->stream_t); if (rcw != RVIO_OK) return rcw; }   // filter(k-2) has consumed hb_imu[b]
        else if (!h->piped) HIPCHK(h, hipStreamSynchronize(h->stream));
        if (m > 0) HIPCHK(h, hipMemcpyAsync(h->hb_imu[b], pp + h->pin_imu, sizeof(rvio_imu) * m, hipMemcpyHostToDevice, h->stream_t));
        HIPCHK(h, hipEventRecord(h->evIn[b], h->stream_t));                                  // propagate (filter stream) only needs the IMU batch
        HIPCHK(h, hipMemcpyAsync(h->hb_img[b], pp, npx, hipMemcpyHostToDevice, h->stream_t));
        if (nc > 0) HIPCHK(h, hipMemcpyAsync(h->hb_cand[b], pp + pin_cand, sizeof(float) * 2 * nc, hipMemcpyHostToDevice, h->stream_t));
        HIPCHK(h, hipEventRecord(h->evPin[ps], h->stream_t));
    }
    h->last_ra = ra;
    if (paranoid_bits() & PAR_SYNC_COPIES) {   // the staging copies have landed before anything that reads them is enqueued
        HIPCHK(h, hipStreamSynchronize(h->stream_d));
        HIPCHK(h, hipStreamSynchronize(h->stream_t));
        if (h->stream_c) HIPCHK(h, hipStreamSynchronize(h->stream_c));
    }
    return frame_dev_impl(h, f, h->hb_img[b], (int)rowb, h->hb_imu[imu_slot], m, cand_xy ? h->hb_cand[b] : nullptr, nc, true);
}
// direct-track variant of the whole frame (host inputs)
int rvio_hip_frame_points(rvio_hip* h, const float* tracked_xy, const unsigned char* status, int n_pts,
                          const rvio_imu* imu, int m, const float* cand_xy, int n_cand) {
    int rc = rvio_hip_track_points(h, tracked_xy, status, n_pts, imu, m, cand_xy, n_cand);
    if (rc != RVIO_OK) return rc;
    return frame_tail_dev(h, h->d_imu, m);
}

int rvio_hip_get_frame_info(rvio_hip* h, rvio_frame_info* info) {
    if (!h || !info) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    SYNC_FRONT(h);   // image / side / tracker streams first
    FilterMeta m;
    double lit_rank = -1.0;
    HIPCHK(h, hipMemcpyAsync(info, h->d_info, sizeof *info, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&m, h->meta, sizeof m, hipMemcpyDeviceToHost, h->stream));
    if (h->last_Ab) HIPCHK(h, hipMemcpyAsync(&lit_rank, h->last_Ab + (size_t)h->dc.ldh * (h->dc.ldh - 1) + 5, sizeof lit_rank, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    info->n_clones = h->n_clones_host; info->n_feat_accepted = m.n_good; info->n_rows = m.n_rows; info->updated = m.updated;
    info->reserved[0] = m.err;
    info->reserved[1] = (m.updated && lit_rank >= 0) ? (int)lit_rank : -1;
    info->rank_truncated_at = m.updated ? m.trunc_at : -1;
    if (m.err & 4) { h->err = "a device-side stage counter timed out (filter -> book-keeping): the frame sequence is invalid, re-initialise"; return RVIO_ERR_STATE; }
    return RVIO_OK;
}
// one instance of a batch handle: augcomp_kernel2 writes d_pose at the slab stride
int rvio_hip_get_pose_at(rvio_hip* h, int instance, double p[3], double q[4]) {
    if (!h || instance < 0 || instance >= h->batch) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    double buf[8];
    HIPCHK(h, hipMemcpyAsync(buf, (const char*)h->d_pose + (size_t)instance * h->slab_bytes, sizeof buf, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (p) for (int i = 0; i < 3; ++i) p[i] = buf[i];
    if (q) for (int i = 0; i < 4; ++i) q[i] = buf[3 + i];
    return RVIO_OK;
}
int rvio_hip_get_pose(rvio_hip* h, double p[3], double q[4]) { return rvio_hip_get_pose_at(h, 0, p, q); }

}  // extern "C"

// ------------------------------------------------------------------ diagnostics for parity tests
extern "C" {
// output of the device detector for the most recent image: corner count, refined corners, goodFeaturesToTrack corners
// before cornerSubPix, and the min-eigenvalue map (each pointer may be NULL)
int rvio_hip_get_corners(rvio_hip* h, int32_t* n, float* xy, float* raw_xy, float* eig) {
    if (!h) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    if (!h->det_ready) { h->err = "the device detector has not run (pass a NULL corner list to track/frame)"; return RVIO_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    SYNC_FRONT(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int cnt = 0;
    HIPCHK(h, hipMemcpyAsync(&cnt, h->det_nout + h->last.dslot, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n) *n = cnt;
    if (xy && cnt > 0) HIPCHK(h, hipMemcpyAsync(xy, h->det_xy2[h->last.dslot], sizeof(float) * 2 * cnt, hipMemcpyDeviceToHost, h->stream));
    const DetDev& ds_ = h->dets[h->last.det_set];
    if (raw_xy && cnt > 0) HIPCHK(h, hipMemcpyAsync(raw_xy, ds_.raw_xy, sizeof(float) * 2 * cnt, hipMemcpyDeviceToHost, h->stream));
    if (eig) {
        // the pipeline no longer stores the min-eigenvalue map (mineig_nms_kernel keeps it in LDS): recomputed on demand from the image the
        // detector saw — level 0 of the current pyramid — by the map-only kernel (same arithmetic); its side effects on the detector's
        // per-frame scratch are undone (the image maximum returns to its rest value)
        const DevCfg& d = h->dc;
        if (!h->eig_map) RCCHK(own_dev(h, &h->eig_map, sizeof(float) * d.W * d.H, true));
        DetDev dm = ds_;
        dm.eig = h->eig_map;
        hipLaunchKernelGGL(mineig_kernel, dim3((d.W + DET_TW - 1) / DET_TW, (d.H + DET_TH - 1) / DET_TH, 1), dim3(DET_T), 0, h->stream, h->pyr[h->pyr_cur].img[0], d.W, dm, (size_t)0,
                           (size_t)0, 0);
        const int rest = (int)0x80000000;
        HIPCHK(h, hipMemcpyAsync(ds_.maxkey, &rest, sizeof rest, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(eig, h->eig_map, sizeof(float) * d.W * d.H, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}
// pyramid level `level` of the most recent image: u8 image (w*h) and int16 (dx,dy) derivative (w*h*2)
int rvio_hip_debug_pyramid(rvio_hip* h, int level, int32_t* w, int32_t* hgt, uint8_t* img, int16_t* dxy) {
    if (!h || level < 0 || level >= h->dc.levels) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    SYNC_FRONT(h);   // image / side / tracker streams first
    const PyrDev& p = h->pyr[h->pyr_cur];
    if (w) *w = p.w[level];
    if (hgt) *hgt = p.h[level];
    const size_t n = (size_t)p.w[level] * p.h[level];
    if (img) HIPCHK(h, hipMemcpyAsync(img, p.img[level], n, hipMemcpyDeviceToHost, h->stream));
    if (dxy) {   // calcSharrDeriv of that level, computed on demand (the pipeline keeps no derivative image)
        OwnedScope tmps(h);
        int* tmp = nullptr;
        RCCHK(tmps.dev(&tmp, n * sizeof(int)));
        hipLaunchKernelGGL(scharr_debug_kernel, dim3((p.w[level] + 63) / 64, (p.h[level] + 3) / 4), dim3(256), 0, h->stream, p.img[level], p.w[level], p.h[level], tmp);
        HIPCHK(h, hipMemcpyAsync(dxy, tmp, n * 2 * sizeof(int16_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}
// raw vFeatsTracked of the last track() call (n entries = mnFeatsToTrack that entered the call)
int rvio_hip_debug_tracked(rvio_hip* h, int n, float* xy, float* un_xy) {
    if (!h || n < 0 || n > h->dc.F) return RVIO_ERR_INVALID;
    FRONT_END_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    SYNC_FRONT(h);   // image / side / tracker streams first
    if (n > 0 && xy) HIPCHK(h, hipMemcpyAsync(xy, h->t.tracked, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, h->stream));
    if (n > 0 && un_xy) HIPCHK(h, hipMemcpyAsync(un_xy, h->t.un2, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}
// Average device time (microseconds, HIP events on the handle's stream) of `iters` back-to-back launches of one
// hot kernel on the operands left behind by the last frame: which = 0 -> solve kernel (W = T^-1 + injection),
// 1 -> klt_kernel3 on the two resident pyramids, 2 -> feat_build_kernel.  Outputs land in scratch / are idempotent.
int rvio_hip_debug_time_kernel(rvio_hip* h, int which, int iters, float* avg_us) {
    if (!h || !avg_us || iters < 1 || which < 0 || which > 15) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    { const int rcd = drain_all(h); if (rcd != RVIO_OK) return rcd; }   // (every queue of the handle: the run-ahead image chains too)
    const DevCfg& d = h->dc;
    const int n = h->n_clones_host;
    // what this handle cannot time, ahead of everything the hook creates
    const bool front_hook = which == 1 || which == 6 || which == 9 || which == 11;
    if (front_hook && !h->front_end) { h->err = "this batch handle was created without its front end"; return RVIO_ERR_UNSUPPORTED; }
    if ((which == 1 || which == 6 || which == 9) && h->batch > 1) return RVIO_ERR_UNSUPPORTED;
    if ((which == 6 || which == 9) && !h->det_ready) return RVIO_ERR_UNSUPPORTED;
    if (which == 8 && (h->batch > 1 || !h->plan.fuse_ok || !h->time_imu || n < 1)) return RVIO_ERR_UNSUPPORTED;
    if (which == 10 && !h->lm.count) return RVIO_ERR_UNSUPPORTED;
    if (which == 15 && (!h->lmc || !h->lm.count || h->lm_frame < 0)) { h->err = "no cloud with covariance has been published (rvio_hip_set_landmark_cov, then an update)"; return RVIO_ERR_UNSUPPORTED; }
    if (which == 11 && (h->pix_fmt == RVIO_PIX_MONO8 || !h->last.gray_src)) { h->err = "no colour or raw image has been handed over (rvio_hip_set_image_format)"; return RVIO_ERR_UNSUPPORTED; }
    if (which == 12 && !ring_exists(h, h->odom)) return RVIO_ERR_UNSUPPORTED;
    if (which == 13 || which == 14) {
        if (!ring_exists(h, h->imuo)) return RVIO_ERR_UNSUPPORTED;
        if (which == 14 && !h->imuc.on) { h->err = "the IMU-rate covariance ring is off (rvio_hip_set_imu_odometry_cov)"; return RVIO_ERR_UNSUPPORTED; }
        if (!h->time_imu || h->time_m < 1) { h->err = "no frame has propagated an IMU batch yet"; return RVIO_ERR_UNSUPPORTED; }
    }
    // the hook's temporaries and its two events: released when this scope ends, whichever return ends it
    OwnedScope tmps(h);
    double *bx = nullptr, *bP = nullptr;
    if (which == 8) {   // (the fused launch propagates in place: the state is put aside and restored behind the timed launches)
        RCCHK(tmps.dev(&bx, sizeof(double) * d.xdmax)); RCCHK(tmps.dev(&bP, sizeof(double) * d.dmax * d.dmax));
        HIPCHK(h, hipMemcpyAsync(bx, h->x[h->cur], sizeof(double) * d.xdmax, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(bP, h->P[h->cur], sizeof(double) * d.dmax * d.dmax, hipMemcpyDeviceToDevice, h->stream));
    }
    rvio_odom* odt = nullptr;        // (12: into a slot of its own: the ring stays what the frames wrote)
    if (which == 12) RCCHK(tmps.dev(&odt, sizeof(rvio_odom) * h->batch));
    rvio_imu_pose* ipt = nullptr;    // (13: into a buffer of its own, in the ring's layout: the ring stays what the frames wrote)
    if (which == 13) RCCHK(tmps.dev(&ipt, sizeof(rvio_imu_pose) * (size_t)h->time_m * h->batch));
    rvio_imu_cov* ict = nullptr;     // (14: likewise)
    if (which == 14) RCCHK(tmps.dev(&ict, sizeof(rvio_imu_cov) * (size_t)h->time_m * h->batch));
    LmOut lmt = {nullptr, nullptr, nullptr, nullptr, 0};
    if (which == 10) {   // (into buffers of its own: the getter's cloud stays the last update's)
        RCCHK(lm_alloc(h, &lmt));
        tmps.held.push_back(lmt.count);   // (the one allocation behind the four pointers)
    }
    rvio_landmark_cov* lct = nullptr;   // (15: into records of its own: the getter's stay the last update's)
    if (which == 15) RCCHK(tmps.dev(&lct, sizeof(rvio_landmark_cov) * (size_t)h->dc.Fu * h->batch));
    // the forms the frame's update would get at this window (time what the chain sees: the Cholesky factor rides in the per-feature launch / runs on its own
    // queue; the slab holds the factor of the last update): fw for a whole update, fs for one separately timed stage
    const bool pre = h->plan.solve9_nt && (h->plan.solve9_nt <= 6 || h->plan.chol_queue);
    const UpdateForms fw = forms_at(h, n, pre, true), fs = forms_at(h, n, pre, false);
    // ... and the kernel forms a front-end call with the device detector gets on the last image handed over (1, 6, 9, 11)
    const FrontForms ff = front_hook ? call_forms(h, false, false, h->last.gray_src, h->last.gray_stride, h->last.gray_bs) : FrontForms();
    hipEvent_t e0 = nullptr, e1 = nullptr;
    RCCHK(tmps.event(&e0, hipEventDefault)); RCCHK(tmps.event(&e1, hipEventDefault));
    HIPCHK(h, hipEventRecord(e0, h->stream));
    for (int it = 0; it < iters; ++it) {
        if (which == 12) {   // odom_kernel as augment_compose_dev launches it, on the composed state the last frame left
            launch_odom(h, odt, h->odom.seq);
        } else
        if (which == 13) {   // imu_pose_kernel as the ring launches it: the IMU batch of the last frame (the caller's device buffer must still be alive), the state that frame left
            launch_imu_pose(h, h->stream, h->batch, h->x[h->cur], h->time_imu, h->time_imu_bs, h->time_m, ipt, 0, 1, h->time_m, h->img_count);
        } else
        if (which == 14) {   // imu_cov_kernel as the ring launches it, on the same operands
            launch_imu_cov(h, h->stream, h->batch, h->x[h->cur], h->P[h->cur], h->time_imu, h->time_imu_bs, h->time_m, ict, 0, 1, h->time_m, h->img_count);
        } else
        if (which == 15) {
            // landmark_cov_kernel as the update launches it, on the last update's cloud, hand-over table and (phi, psi, rho); the state and covariance
            // buffers are the ones it reads (behind a whole frame they hold other values — the same arithmetic on the same span)
            launch_landmark_cov(h, n, h->lm, lct);
        } else
        if (which == 10) {
            // landmark_kernel as the update launches it, on the hand-over table, accept flags and (phi, psi, rho) of the last update; the state
            // buffers are the ones it reads (behind a whole frame: the composed state and xk1k1 — the same arithmetic)
            launch_landmarks(h, n, lmt);
        } else
        if (which == 8) {
            // feat_prop_kernel exactly as the pipelined frame launches it: the per-feature workgroups of the last hand-over table + PreIntegrator::propagate on the
            // IMU batch of the last frame (the caller's device buffer must still be alive) + at 6n <= 96 the Cholesky role
            launch_feat_prop(h, n, h->time_imu, h->time_m, 0, 1);
        } else if (which == 9) {   // the detector's selection kernel (one workgroup: priority-ordered maximal independent set) on the candidates of the last detector call
            const DetDev q = det_view(h, h->last.det_set, h->last.dslot);
            hipLaunchKernelGGL(greedy_kernel, lp_grid(ff.greedy_l), lp_block(ff.greedy_l), ff.greedy_l.lds, h->stream, q, h->slab_bytes);
        } else
        if (which == 0) {
            launch_solve(h, fw, n, h->block);   // as the frame's update launches it: dx = Pc y and the state injection are roles of the Joseph launch behind it (not run here)
        } else if (which == 1) {
            // KLT as the frame ran it cannot be repeated (book-keeping has moved the features to where they were tracked): match the CURRENT
            // image back onto the PREVIOUS one from the current feature positions instead — the same displacement magnitudes, reversed, the
            // refilled corners included (they exist in the previous image too).  Outputs land in t.tracked / t.status (scratch between frames).
            // (the form the frames of this handle get: klt_kernel16 once rvio_hip_debug_kernel_forms has switched it to the throughput forms)
            if (ff.klt == LPKL_K16)
                hipLaunchKernelGGL(klt_kernel16, lp_grid(ff.klt_l), lp_block(ff.klt_l), 0, h->stream, h->pyr[h->pyr_cur], h->pyr[(h->pyr_cur + 3) % 4], d.levels, h->t.n_pts, h->t.feats,
                                   h->t.tracked, h->t.status, (size_t)0);
            else
                hipLaunchKernelGGL(klt_kernel3, lp_grid(ff.klt_l), lp_block(ff.klt_l), 0, h->stream, h->pyr[h->pyr_cur], h->pyr[(h->pyr_cur + 3) % 4], d.levels, h->t.n_pts, h->t.feats,
                                   h->t.tracked, h->t.status, (size_t)0, (const unsigned long long*)nullptr, 0ull, h->meta);
        } else if (which == 2) {
            launch_feat_build(h, n, 0, 1);   // (a batch handle: on the pose chains geom4_kernel left in the last update)
        } else if (which == 3) {   // reduction of the per-feature shares + rank truncation (reads `partial`, rewrites `block`: idempotent)
            launch_gram(h, fw, n);
        } else if (which == 4 || which == 5) {   // U, G, P1 strips / the Joseph form on the operands of the last update, in the form the handle launches
            launch_ug_final(h, fs, n, h->block, h->P[h->cur ^ 1], which == 4, which == 5, false);   // (outputs: scratch / the spare covariance buffer, overwritten by the next stage anyway)
        } else if (which == 7) {   // U, G, P1 + the Joseph form as the handle launches them for a whole update (one instance, 6n <= 60: ONE kernel)
            launch_ug_final(h, fw, n, h->block, h->P[h->cur ^ 1], true, true, false);   // (no solve ran ahead of the timed launch: no dx waits for its roles)
        } else if (which == 6) {   // cornerSubPix on the corners of the last detector call (reads raw_xy, rewrites xy with the same values)
            const DetDev q = det_view(h, h->last.det_set, h->last.dslot);
            const uint8_t* im = h->pyr[h->pyr_cur].img[0];   // level 0 of the current pyramid = the image the detector saw
            launch_subpix(h, ff, q, im, d.W, (size_t)0, 0, h->stream);
        } else if (which == 11) {   // gray_kernel on the last image handed over, in the form the frame launched, into the slot it wrote (the same values again)
            launch_gray(h, ff, h->last.gray_src, h->last.gray_stride, h->last.gray_bs, h->d_gray[h->gray_slot], h->stream);
        }
    }
    HIPCHK(h, hipEventRecord(e1, h->stream));
    // the timed solves ran on the slab: the next update factors the clone block itself.  (drain_all() above has synchronised stream_c, which IS
    // stream_l, so a factor that was in flight has landed.)
    if (which == 0) (void)chol_drop(h, CHOL_DRAINED);
    if (which == 8) {
        HIPCHK(h, hipMemcpyAsync(h->x[h->cur], bx, sizeof(double) * d.xdmax, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->P[h->cur], bP, sizeof(double) * d.dmax * d.dmax, hipMemcpyDeviceToDevice, h->stream));
        chol_role(h, false);   // (what the role workgroups of the timed launches left is not kept.  No chol_drop: P is again what it was, a factor from stream_l stays its factor)
    }
    HIPCHK(h, hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1e3f / iters;
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}

// Test hook against results that depend on LEFT-OVER state: every stream is drained, then
//   what & 1   the filter's scratch — per-feature shares, information block, T, W, U, G, the d x d temporary, the gate's diagnostics, and the
//              SPARE state / covariance buffer (every stage writes its output in full) — is filled with 0xff bytes (NaN doubles, -1 ints)
//   what & 2   a kernel of 160 KB workgroups rewrites the LDS of the whole chip with signalling-NaN patterns
//   what & 4   the Tracker -> Updater hand-over tables (types / len / meas of all kHand tables; the counts stay) and the tracker's per-frame
//              scratch (vFeatsTracked, vFeatsUndistNorm, the next-frame order being built, FindNewer flags, ChessGrid cells) likewise
//   what & 8   sets the device-side error bit 4 ("a stage counter timed out"): the recovery path through rvio_hip_initialize can be tested
// A frame sequence must give the same results with any of 1 | 2 | 4 between its frames (tests/test_gpu_leftover.py).
__global__ __launch_bounds__(256) void lds_poison_kernel(unsigned long long pattern, int* sink) {
    extern __shared__ __align__(16) unsigned long long lp[];
    const int nw = 160 * 1024 / 8;
    for (int i = threadIdx.x; i < nw; i += 256) lp[i] = pattern ^ (unsigned long long)i;
    __syncthreads();
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < 2000) __builtin_amdgcn_s_sleep(8);   // 20 us: long enough for every CU to be handed a workgroup
    if (lp[(threadIdx.x * 977) % nw] == 1ull && sink) *sink = 1;      // (keeps the stores alive)
}
int rvio_hip_debug_poison(rvio_hip* h, int what) {
    if (!h) return RVIO_ERR_INVALID;
    { const int rc = drain_all(h); if (rc != RVIO_OK) return rc; }
    const DevCfg& d = h->dc;
    const size_t dm = d.dmax, PP = dm * dm, ldh = d.ldh;
    auto fill = [&](void* p, size_t bytes) -> hipError_t {
        if (!p || !bytes) return hipSuccess;
        hipError_t e = hipSuccess;
        for (int z = 0; z < h->batch && e == hipSuccess; ++z) e = hipMemsetAsync((char*)p + (size_t)z * h->slab_bytes, 0xff, bytes, h->stream);
        return e;
    };
    if (what & 1) {
        HIPCHK(h, fill(h->partial, sizeof(double) * d.Fu * ldh * ldh));
        HIPCHK(h, fill(h->block, sizeof(double) * 2 * ldh * ldh)); HIPCHK(h, fill(h->Ab, sizeof(double) * 2 * ldh * ldh));
        HIPCHK(h, fill(h->Tbuf, sizeof(double) * ldh * ldh)); HIPCHK(h, fill(h->W, sizeof(double) * ldh * ldh));
        if (h->S9scr) {   // the slab holds the Cholesky factor a PRE solve would read (role workgroup / stream_l): it goes with the slab — the next solve factors Pcc itself
            HIPCHK(h, hipMemsetAsync(h->S9scr, 0xff, sizeof(double) * S9_SLAB_DOUBLES(h->plan.solve9_nt), h->stream));
            (void)chol_drop(h, CHOL_DRAINED);   // (drain_all above has waited for stream_l)
        }
        HIPCHK(h, fill(h->U, sizeof(double) * dm * ldh)); HIPCHK(h, fill(h->G, sizeof(double) * dm * ldh));
        HIPCHK(h, fill(h->Pt1, sizeof(double) * PP));
        HIPCHK(h, fill(h->gamma, sizeof(double) * d.Fu)); HIPCHK(h, fill(h->pfinv, sizeof(double) * 3 * d.Fu));
        HIPCHK(h, fill(h->nrows, sizeof(int) * d.Fu)); HIPCHK(h, fill(h->acc, sizeof(int) * d.Fu)); HIPCHK(h, fill(h->ndof, sizeof(int) * d.Fu));
        if (h->tm_global) HIPCHK(h, fill(h->tm_global, sizeof(double) * d.Fu * d.rho_max * ldh));
        if (h->gpose) { HIPCHK(h, fill(h->gpose, sizeof(double) * d.Fu * (d.max_len - 1) * 24)); HIPCHK(h, fill(h->gvalid, sizeof(int) * d.Fu)); }
        HIPCHK(h, fill(h->x[h->cur ^ 1], sizeof(double) * d.xdmax)); HIPCHK(h, fill(h->P[h->cur ^ 1], sizeof(double) * PP));
    }
    if ((what & 4) && h->front_end) {
        const TrackerDev& t = h->t;
        for (int k = 0; k < rvio_hip::kHand; ++k) {
            HIPCHK(h, fill(h->tout[k].types, d.Fu)); HIPCHK(h, fill(h->tout[k].len, sizeof(int) * d.Fu));
            HIPCHK(h, fill(h->tout[k].meas, sizeof(float) * 2 * d.Fu * d.max_len));
        }
        HIPCHK(h, fill(t.tracked, sizeof(float) * 2 * d.F)); HIPCHK(h, fill(t.un2, sizeof(float) * 2 * d.F));
        HIPCHK(h, fill(t.tmp_feats, sizeof(float) * 2 * d.F)); HIPCHK(h, fill(t.tmp_un, sizeof(float) * 2 * d.F)); HIPCHK(h, fill(t.tmp_slot, sizeof(int) * d.F));
        HIPCHK(h, fill(t.cand_acc, sizeof(int) * d.F));
        HIPCHK(h, fill(t.cell_pts, sizeof(float) * (size_t)d.grid_cols * d.grid_rows * 2 * d.F * 2));
        if (h->d_gray[0]) HIPCHK(h, hipMemsetAsync(h->d_gray[0], 0xff, 4 * (size_t)d.W * d.H * h->batch, h->stream));   // (one allocation: every slot of every instance)
    }
    if (what & 2) {
        static bool attr = false;
        if (!attr) { HIPCHK(h, lds_attr((const void*)lds_poison_kernel, 160 * 1024)); attr = true; }
        hipLaunchKernelGGL(lds_poison_kernel, dim3(1024), dim3(256), 160 * 1024, h->stream, 0x7ff4dead00000000ull, (int*)nullptr);
        HIPCHK(h, hipGetLastError());
    }
    if (what & 8) {
        const int four = 4;   // (|= 4 on a drained handle: read-modify-write through the host)
        int e = 0;
        HIPCHK(h, hipMemcpyAsync(&e, &h->meta->err, sizeof e, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        e |= four;
        HIPCHK(h, hipMemcpyAsync(&h->meta->err, &e, sizeof e, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RVIO_OK;
}

// Test hook against ordering holes between the handle's streams: a one-wave kernel that occupies `which` (0 filter stream, 1 tracker /
// image chain 0, 2 side stream: KLT, RANSAC, book-keeping, 3 image chain 1) for `usec` microseconds, enqueued where the call is made.
// Every dependency of the pipeline has to hold under ANY pacing of its queues, so a frame sequence with stalls sprinkled over its streams
// must give the results of the synchronised run bit for bit (tests/test_gpu_flatout.py) — independent of how fast the box happens to be.
__global__ __launch_bounds__(64) void stall_kernel(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
int rvio_hip_debug_stall(rvio_hip* h, int which, int usec) {
    if (!h || which < 0 || which > 3 || usec < 0 || usec > 1000000) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = which == 0 ? h->stream : which == 1 ? h->stream_t : which == 2 ? h->stream_d : h->stream_c;
    if (!st) return RVIO_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(stall_kernel, dim3(1), dim3(64), 0, st, (unsigned long long)usec * 100ull);   // the constant 100 MHz clock
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}

// Test hook against timing dependence INSIDE kernels (cross-wave hand-overs through LDS flags, last-block patterns, atomics): `wgs`
// workgroups on a stream of their own hammer HBM, L2 and LDS for `usec` microseconds beside whatever the handle has in flight — a box
// under load.  Waves of the pipeline's kernels then share SIMDs, LDS ports and L2 slices with the noise and run at a different relative
// pace; not one bit of any result may move (tests/test_gpu_flatout.py).
__global__ __launch_bounds__(256) void noise_kernel(unsigned long long ticks, double* scratch, size_t n_per_wg) {
    __shared__ double sh[4096];
    double* g = scratch + (size_t)blockIdx.x * n_per_wg;
    for (int i = threadIdx.x; i < 4096; i += 256) sh[i] = (double)i;
    __syncthreads();
    const unsigned long long t0 = wall_clock64();
    double acc = 0;
    unsigned it = 0;
    while (wall_clock64() - t0 < ticks) {
        for (size_t i = threadIdx.x; i < n_per_wg; i += 256) { const double v = g[i] + sh[(i + it) & 4095]; g[i] = v * 0.999; acc += v; }
        sh[(threadIdx.x * 17 + it) & 4095] = acc;
        __syncthreads();
        ++it;
    }
    if (acc == 1.2345e300) g[0] = acc;
}
int rvio_hip_debug_kernel_forms(rvio_hip* h, int throughput) {
    if (!h) return RVIO_ERR_INVALID;
    h->wide_px = throughput != 0;
    return RVIO_OK;
}
int rvio_hip_debug_noise(rvio_hip* h, int wgs, int usec) {
    if (!h || wgs < 1 || wgs > 4096 || usec < 0 || usec > 1000000) return RVIO_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    static hipStream_t ns = nullptr;
    static double* scratch = nullptr;
    const size_t per = 8192;   // 64 KB per workgroup: L2-resident for a few hundred workgroups, HBM beyond
    if (!ns) {
        HIPCHK(h, hipStreamCreateWithFlags(&ns, hipStreamNonBlocking));
        HIPCHK(h, hipMalloc((void**)&scratch, sizeof(double) * per * 4096));
        HIPCHK(h, hipMemset(scratch, 0, sizeof(double) * per * 4096));
    }
    hipLaunchKernelGGL(noise_kernel, dim3(wgs), dim3(256), 0, ns, (unsigned long long)usec * 100ull, scratch, per);
    HIPCHK(h, hipGetLastError());
    return RVIO_OK;
}

int rvio_hip_debug_ring(rvio_hip* h, long long* out512, int* frame) {
    if (!h || !out512 || !frame) return RVIO_ERR_INVALID;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpyFromSymbol(out512, HIP_SYMBOL(g_ring), sizeof(long long) * 512));
    HIPCHK(h, hipMemcpyFromSymbol(frame, HIP_SYMBOL(g_ring_frame), sizeof(int)));
    return RVIO_OK;
}
int rvio_hip_debug_ring2(rvio_hip* h, long long* out512, int* frame) {
    if (!h || !out512 || !frame) return RVIO_ERR_INVALID;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpyFromSymbol(out512, HIP_SYMBOL(g_ring2), sizeof(long long) * 512));
    HIPCHK(h, hipMemcpyFromSymbol(frame, HIP_SYMBOL(g_ring2_frame), sizeof(int)));
    return RVIO_OK;
}
int rvio_hip_debug_ring3(rvio_hip* h, long long* out512) {
    if (!h || !out512) return RVIO_ERR_INVALID;
    int rc = rvio_hip_sync(h);
    if (rc != RVIO_OK) return rc;
    HIPCHK(h, hipMemcpyFromSymbol(out512, HIP_SYMBOL(g_ring3), sizeof(long long) * 512));
    return RVIO_OK;
}
// experiments (tools/at_rest_literal.py): every update the literal sweep can take takes it (process-wide switch)
int rvio_hip_debug_literal_force(rvio_hip* h, int on) {
    if (!h) return RVIO_ERR_INVALID;
    const int rc = drain_all(h);
    if (rc != RVIO_OK) return rc;
    const int v = on ? 1 : 0;
    HIPCHK(h, hipMemcpyToSymbol(HIP_SYMBOL(g_lit_force), &v, sizeof v));
    return RVIO_OK;
}
int rvio_hip_debug_clocks2(rvio_hip* h, long long* out64) {
    if (!h || !out64) return RVIO_ERR_INVALID;
    const int rc = drain_all(h);
    if (rc != RVIO_OK) return rc;
    HIPCHK(h, hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_dbg2), sizeof(long long) * 64));
    return RVIO_OK;
}
// the per-phase sums / counts of feat_build_body over all workgroups (DBG_P) into out64, the longest phases (g_dbg2[30..40]) into max64; both cleared
int rvio_hip_debug_phases(rvio_hip* h, long long* out64, long long* max64) {
    if (!h || !out64 || !max64) return RVIO_ERR_INVALID;
    const int rc = drain_all(h);
    if (rc != RVIO_OK) return rc;
    static const long long zero[64] = {0};
    HIPCHK(h, hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_dbg3), sizeof(long long) * 64));
    HIPCHK(h, hipMemcpyFromSymbol(max64, HIP_SYMBOL(g_dbg2), sizeof(long long) * 64));
    HIPCHK(h, hipMemcpyToSymbol(HIP_SYMBOL(g_dbg3), zero, sizeof zero));
    HIPCHK(h, hipMemcpyToSymbol(HIP_SYMBOL(g_dbg2), zero, sizeof zero));
    return RVIO_OK;
}
int rvio_hip_debug_clocks(rvio_hip* h, long long* out64) {
    if (!h || !out64) return RVIO_ERR_INVALID;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_dbg), sizeof(long long) * 64));
    return RVIO_OK;
}
}
