/*
 * rvio_hip.h — C-ABI of the MI355X-native robocentric MSCKF hot path.
 *
 * The reference (rpng/R-VIO) has no FFI/plugin layer: its per-frame hot path
 * sits behind three C++ member calls made from System::MonoVIO
 * (src/rvio/System.cc:258,263,268).  Each entry point below replaces one of
 * those calls (or a slice of MonoVIO itself) and cites it.  Everything is
 * POD + plain pointers; no C++/torch types cross this boundary.
 *
 * Conventions
 *   - state vector x  : [qG(4) pG(3) g(3) | qk(4) pk(3) v(3) bg(3) ba(3) | n x (q(4) p(3))]
 *                       JPL quaternions [x y z w]   (System.cc:142-149,326-331)
 *   - covariance  P   : (24+6n)^2 doubles, COLUMN-major (Eigen::MatrixXd layout),
 *                       error state [thG pG g | thk pk v bg ba | n x (th p)]
 *   - all functions return RVIO_OK (0) or a negative rvio_status; the silent
 *     early-outs of the reference (too few features etc.) are reported through
 *     rvio_frame_info, not through the return code.
 *   - a handle owns one HIP stream and all device memory of one filter
 *     instance; a handle is not thread-safe, distinct handles are independent.
 *   - functions ending in _dev take DEVICE pointers, all others HOST pointers.
 *   - every entry point is asynchronous on the handle's stream unless it
 *     returns data to host memory (get_* / *_sync), which synchronise.
 */
#ifndef RVIO_HIP_H
#define RVIO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVIO_HIP_ABI_VERSION 6   /* 3: rvio_hip_frame_sharded_dev, IMU batches of any length, error bits 4 (hard) / 8;  4: the rvio_hip_debug_poison / _stall / _noise / _kernel_forms test hooks are part of the exported surface;  5: the payload of rvio_hip_update_local / _global is the packed wire format of csrc/rvio_dev.h shard_layout;  6: the landmark cloud (rvio_hip_set_landmarks, rvio_hip_get_landmarks, rvio_hip_get_landmarks_at);  added WITHIN 6, purely additive (no struct, no existing prototype changed): rvio_hip_set_image_format, rvio_hip_get_image_format; the odometry ring (rvio_odom, rvio_hip_set_odometry, rvio_hip_get_odometry, rvio_hip_get_odometry_all) and rvio_hip_get_pose_at; per-instance calibration (rvio_calibration, rvio_calibration_from_config, rvio_hip_set_calibration_at, rvio_hip_set_calibrations, rvio_hip_get_calibration_at) and rvio_hip_initialize_at; IMU-rate odometry (rvio_imu_pose, rvio_hip_predict, rvio_hip_predict_dev, rvio_hip_set_imu_odometry, rvio_hip_get_imu_odometry); the auxiliary measurement update (rvio_aux_meas, rvio_aux_mode, rvio_hip_update_aux, rvio_hip_update_aux_dev, rvio_hip_get_aux_diag); the covariance of IMU-rate odometry (rvio_imu_cov, rvio_hip_predict_cov, rvio_hip_predict_cov_dev, rvio_hip_set_imu_odometry_cov, rvio_hip_get_imu_odometry_cov); standstill detection (rvio_standstill_config, rvio_standstill, rvio_standstill_config_default, rvio_hip_set_standstill, rvio_hip_standstill, rvio_hip_standstill_dev, rvio_hip_get_standstill); absolute fixes (rvio_fix_kind, rvio_fix, rvio_fix_diag, rvio_hip_update_fix, rvio_hip_update_fix_dev, rvio_hip_get_fix, rvio_hip_get_fix_rows); past-frame fixes (rvio_hip_update_fix_past, rvio_hip_update_fix_past_dev, rvio_hip_frame_age); relative-pose measurements (rvio_rel_kind, rvio_hip_update_rel, rvio_hip_update_rel_dev); map landmarks (rvio_map_units, rvio_map_obs, rvio_map_point, rvio_map_diag, rvio_hip_update_map, rvio_hip_update_map_dev, rvio_hip_get_map, rvio_hip_get_map_rows); iterated measurement updates (rvio_meas_iter, rvio_hip_set_meas_iterations, rvio_hip_get_meas_iterations, rvio_hip_get_meas_iter); landmark covariance (rvio_landmark_cov, rvio_hip_set_landmark_cov, rvio_hip_get_landmark_cov, rvio_hip_get_landmark_cov_at, rvio_hip_get_landmark_cov_dev) */
/* IMU samples the staging of the host-buffer entry points is allocated for (0.96 s at 200 Hz).  PreIntegrator::propagate iterates any
 * list (PreIntegrator.cc:96-97), and so does every entry point here: a longer batch (dropped images) is accepted — the staging grows once,
 * at the price of one host synchronisation; the _dev entry points take any m. */
#define RVIO_HIP_MAX_IMU 192

typedef enum rvio_status {
    RVIO_OK = 0,
    RVIO_ERR_INVALID = -1,     /* bad argument / size                                   */
    RVIO_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime error (see last_error)    */
    RVIO_ERR_UNSUPPORTED = -3, /* e.g. Tracker.nMinDist >= 128 with the device detector (cornerSubPix half-windows 1..63) */
    RVIO_ERR_STATE = -4        /* call out of sequence (e.g. update before set_state)    */
} rvio_status;

/* All parameters of config/rvio_euroc.yaml that the hot path consumes
 * (key -> consumer table: SURVEY.md appendix A).  Types mirror what the
 * reference stores them as (float32 intrinsics: Tracker.cc:39-62; float32
 * sigma_im: Updater.cc:42-44). */
typedef struct rvio_config {
    /* IMU.*  (PreIntegrator.cc:32-44, System.cc:60-67) */
    double imu_rate;      /* IMU.dps          */
    double sigma_g;       /* IMU.sigma_g      */
    double sigma_wg;      /* IMU.sigma_wg     */
    double sigma_a;       /* IMU.sigma_a      */
    double sigma_wa;      /* IMU.sigma_wa     */
    double gravity;       /* IMU.nG           */
    double small_angle;   /* IMU.nSmallAngle  */
    /* Camera.* */
    int32_t width, height;            /* FeatureDetector.cc:37-38               */
    float fx, fy, cx, cy;             /* Tracker.cc:39-42                       */
    float k1, k2, p1, p2, k3;         /* Tracker.cc:51-61                       */
    float sigma_px, sigma_py;         /* Updater.cc:42-44 (sigma_im = max)      */
    double T_bc[16];                  /* Camera.T_BC0, ROW-major 4x4 (Updater.cc:46-53) */
    int32_t fisheye;                  /* Camera.Fisheye: cv::fisheye::undistortPoints with D = (k1,k2,p1,p2) (Tracker.cc:116-119) */
    /* Tracker.* */
    int32_t n_features;               /* Tracker.nFeatures          (Tracker.cc:73)  supported: 2 .. 4096 (ceil(n/2) <= 2048 hand-over slots);
                                         beyond it create returns RVIO_ERR_UNSUPPORTED and rvio_hip_last_error names the limit.  Every count in
                                         the range is created and launched: book-keeping runs with as many waves as one CU's LDS holds beside
                                         the kernel's static LDS, and as two launches instead of one above 2850 */
    int32_t max_track_len;            /* Tracker.nMaxTrackingLength (Tracker.cc:78)  supported: 3 .. 32 */
    int32_t min_track_len;            /* Tracker.nMinTrackingLength (Tracker.cc:79)  >= 2 */
    float   min_dist;                 /* Tracker.nMinDist           (FeatureDetector.cc:31) */
    float   qual_lvl;                 /* Tracker.nQualLvl           */
    float   block_x, block_y;         /* Tracker.nBlockSizeX/Y, stored as float like upstream (FeatureDetector.h:72-73) */
    int32_t enable_equalizer;         /* Tracker.EnableEqualizer    (Tracker.cc:70-71) */
    int32_t use_sampson;              /* Tracker.UseSampson         (Ransac.cc:34-35) */
    double  inlier_thr;               /* Tracker.nInlierThrd        (Ransac.cc:37)    */
    /* INI.* (System.cc:77-91) */
    double  ini_thr_angle;            /* INI.nThresholdAngle */
    double  ini_thr_displ;            /* INI.nThresholdDispl */
    int32_t ini_enable_alignment;     /* INI.EnableAlignment */
    int32_t reserved0;
} rvio_config;

/* Fill *cfg with the stock values of config/rvio_euroc.yaml:8-111. */
void rvio_config_euroc(rvio_config* cfg);

/* One IMU sample: struct ImuData (InputBuffer.h:35-51). */
typedef struct rvio_imu {
    double w[3];   /* AngularVel   */
    double a[3];   /* LinearAccel  */
    double t;      /* Timestamp    */
    double dt;     /* TimeInterval */
} rvio_imu;

/* The Tracker -> Updater hand-over: mvFeatTypesForUpdate + mvlFeatMeasForUpdate
 * (Tracker.h:67-74), flattened.  meas[f][k] is the k-th (oldest first)
 * undistorted-normalised observation (cv::Point2f) of feature f. */
typedef struct rvio_tracks {
    int32_t n_feat;              /* mvFeatTypesForUpdate.size()                 */
    int32_t max_len;             /* row stride of meas, >= every len[f]         */
    const unsigned char* types;  /* n_feat x '1' (lost) | '2' (max length)      */
    const int32_t* len;          /* n_feat track lengths                        */
    const float* meas;           /* n_feat x max_len x 2 float32                */
} rvio_tracks;

/* What the reference only logs through ROS_DEBUG, made observable. */
typedef struct rvio_frame_info {
    int32_t n_clones;          /* nCloneStates after the frame                  */
    int32_t n_tracked_in;      /* mnFeatsToTrack entering track()               */
    int32_t n_klt_ok;          /* status!=0 after KLT                           */
    int32_t n_ransac_inliers;  /* FindInliers return value                      */
    int32_t n_feat_update;     /* features handed to update()                   */
    int32_t n_feat_accepted;   /* nGoodFeatCount                                */
    int32_t n_rows;            /* stacked rows nRowCount                        */
    int32_t updated;           /* 1 if the EKF update was applied               */
    int32_t n_tracked_out;     /* mnFeatsToTrack leaving track() (after refill) */
    int32_t ransac_winner;     /* nWinnerHypothesisIdx                          */
    int32_t reserved[5];       /* [0]: sticky device-side error flag: 1 = singular pivot in the solve, 2 = a track the window cannot hold was
                                * dropped, 4 = a device-side stage counter (filter done -> book-keeping) timed out,
                                * 8 = a non-positive pivot in a feature's gate matrix S_f (indefinite covariance handed in): that feature was rejected
                                * [1]: nRank of the reference's literal Givens sweep + leading-row scan (Updater.cc:493-523) when this update ran it on the
                                * device (an update of a handful of features whose rank decision the structure of the stack does not settle), -1 otherwise */
    int32_t rank_truncated_at; /* Updater.cc:516-529: nRank when the leading-row scan cut informative rows off (the type-'1'
                                * features' rows, dropped from this update), -1 otherwise */
} rvio_frame_info;

typedef struct rvio_hip rvio_hip;  /* opaque; replaces the System-owned stage objects (System.h:89-92) */

/* --- lifetime ------------------------------------------------------------- */
/* new Tracker/Updater/PreIntegrator (System.cc:96-99).  device = HIP ordinal. */
int rvio_hip_create(const rvio_config* cfg, int device, rvio_hip** out);
void rvio_hip_destroy(rvio_hip* h);
const char* rvio_hip_last_error(const rvio_hip* h);
int rvio_hip_abi_version(void);
/* the hipStream_t (as void*) all work of this handle is enqueued on */
void* rvio_hip_stream(rvio_hip* h);
int rvio_hip_sync(rvio_hip* h);

/* --- filter state --------------------------------------------------------- */
/* System::xkk / Pkk (System.h:85-86).  xdim = 26+7n, d = 24+6n. */
int rvio_hip_set_state(rvio_hip* h, const double* x, int xdim, const double* P, int d);
int rvio_hip_get_state(rvio_hip* h, double* x, int* xdim, double* P, int* d);
/* System::initialize (System.cc:115-170): gravity-aligned x(26), P(24x24). */
int rvio_hip_initialize(rvio_hip* h, const double w[3], const double a[3], int n_imu);

/* --- stage entry points (one per reference call site) ---------------------- */
/* PreIntegrator::propagate (PreIntegrator.h:40, call site System.cc:263).
 * Mutates the handle's (x,P) in place: they become xk1k / Pk1k. */
int rvio_hip_propagate(rvio_hip* h, const rvio_imu* imu, int m);

/* Updater::update (Updater.h:43-44, call site System.cc:268) on host-provided
 * tracks.  (x,P) become xk1k1 / Pk1k1; pass-through if <=2 features survive
 * (Updater.cc:460,621-627). */
int rvio_hip_update(rvio_hip* h, const rvio_tracks* tracks);

/* State augmentation + window slide + robocentric composition
 * (System.cc:279-365).  do_augment mirrors `nImageCountAfterInit>1`. */
int rvio_hip_augment_compose(rvio_hip* h, int do_augment);

/* --- visual front end ------------------------------------------------------ */
/* Tracker::track (Tracker.h:50, call site System.cc:258) on a W x H u8 image (interleaved colour pixels: rvio_hip_set_image_format).
 * `cand`/`n_cand` are the detector's corner list for this frame, i.e. the
 * output of FeatureDetector::DetectWithSubPix (FeatureDetector.cc:55-75; the
 * detector itself is outside the hot path); the grid-based
 * selection FindNewer (FeatureDetector.cc:97-150) and the refill
 * (Tracker.cc:344-387) run on the device.  Results stay on the device for
 * rvio_hip_update_tracked and can be fetched with rvio_hip_get_tracks. */
int rvio_hip_track(rvio_hip* h, const uint8_t* img, int stride,
                   const rvio_imu* imu, int m, const float* cand_xy, int n_cand);
int rvio_hip_track_dev(rvio_hip* h, const uint8_t* d_img, int stride,
                       const rvio_imu* d_imu, int m, const float* d_cand_xy, int n_cand);
/* Direct-track mode: the caller supplies the result of the
 * calcOpticalFlowPyrLK call (vFeatsTracked, vInlierFlag; Tracker.cc:244) for the
 * n_pts currently tracked features; everything after Tracker.cc:246 (undistort,
 * RANSAC, book-keeping, refill) runs on the device as in rvio_hip_track. */
int rvio_hip_track_points(rvio_hip* h, const float* tracked_xy, const unsigned char* status, int n_pts,
                          const rvio_imu* imu, int m, const float* cand_xy, int n_cand);
/* Corner lists.  Every image entry point (rvio_hip_track, rvio_hip_track_dev, rvio_hip_frame,
 * rvio_hip_frame_dev) accepts cand_xy == NULL: the library then runs
 * FeatureDetector::DetectWithSubPix (FeatureDetector.cc:55-75: goodFeaturesToTrack with
 * s*nMinDist, s = 1 on the first image / 2 on refills, + cornerSubPix) on the device, on the image
 * the tracker sees (after CLAHE), concurrently with pyramid/KLT/RANSAC (two streams).  A non-NULL list
 * replaces the detector (caller-side detection).  rvio_hip_get_corners copies the device
 * detector's last result out: refined corners, the corners before cornerSubPix and the
 * min-eigenvalue map (W*H floats); each pointer may be NULL. */
int rvio_hip_get_corners(rvio_hip* h, int32_t* n, float* xy, float* raw_xy, float* eig);

/* Pixel format of the images handed to the image entry points: "Convert to gray scale" at the head of Tracker::track
 * (Tracker.cc:182-196: cvtColor with CV_RGB2GRAY / CV_BGR2GRAY for three channels, CV_RGBA2GRAY / CV_BGRA2GRAY for four, chosen by
 * Camera.RGB) on the device.  OpenCV's 8-bit fixed-point form: Y = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14; alpha is ignored. */
typedef enum rvio_pixel_format {
    RVIO_PIX_MONO8 = 0,   /* default: one byte per pixel, nothing is converted */
    RVIO_PIX_RGB8 = 1,    /* three bytes per pixel, R first (Camera.RGB: 1) */
    RVIO_PIX_BGR8 = 2,    /* three bytes per pixel, B first (Camera.RGB: 0) */
    RVIO_PIX_RGBA8 = 3,   /* four bytes per pixel, R first */
    RVIO_PIX_BGRA8 = 4,   /* four bytes per pixel, B first */
    /* Raw sensor data (added within 6): what cv_bridge::toCvShare(msg, MONO8) converts in front of Tracker::track (rvio_mono.cc:64).  Bit 4: 16-bit
     * samples in host byte order (little endian); bit 5: a Bayer mosaic, one sample per pixel, named as ROS does by the top-left 2 x 2 block in
     * reading order (RGGB: (0,0) = R, (1,0) = G, (0,1) = G, (1,1) = B).  Every value that is not listed here is RVIO_ERR_INVALID. */
    RVIO_PIX_MONO16 = 16, /* two bytes per pixel: y8 = (v + 128) / 257, the round-to-nearest of v * 255 / 65535 */
    RVIO_PIX_RGB16 = 17,  /* six bytes per pixel: y16 = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14, then the depth step */
    RVIO_PIX_BGR16 = 18,
    RVIO_PIX_RGBA16 = 19, /* eight bytes per pixel, alpha ignored */
    RVIO_PIX_BGRA16 = 20,
    RVIO_PIX_BAYER_RGGB8 = 32,   /* one byte per pixel: cvtColor's bilinear COLOR_Bayer*2GRAY, borders replicated (the arithmetic: csrc/raw.h) */
    RVIO_PIX_BAYER_BGGR8 = 33,
    RVIO_PIX_BAYER_GBRG8 = 34,
    RVIO_PIX_BAYER_GRBG8 = 35,
    RVIO_PIX_BAYER_RGGB16 = 48,  /* two bytes per pixel: the same formulas on 16-bit samples, then the depth step */
    RVIO_PIX_BAYER_BGGR16 = 49,
    RVIO_PIX_BAYER_GBRG16 = 50,
    RVIO_PIX_BAYER_GRBG16 = 51
} rvio_pixel_format;
/* Off (RVIO_PIX_MONO8) by default: such a handle allocates and launches what it did before these two entry points existed.  With a colour
 * format `img` / `d_img` / `d_imgs` of rvio_hip_track, _track_dev, _frame, _frame_dev, _frame_begin_dev, _frame_sharded_dev and
 * _frame_batch_dev are interleaved pixels; `stride` (and `img_stride`) stay in BYTES, and stride < width * channels is RVIO_ERR_INVALID.
 * One more launch converts the image at the head of the frame's image chain (in front of CLAHE; with the equaliser off in front of the
 * detector and the pyramid) into a gray buffer of the handle, which every later stage reads; the host-buffer entry points stage the
 * caller's colour bytes, no pixel is converted on the host.  A change of format drains the handle and takes effect from the next image
 * handed over; the first colour format allocates the gray buffers.  RVIO_ERR_INVALID: unknown format; RVIO_ERR_UNSUPPORTED: a colour format
 * on a batch handle created without its front end (it takes no image).  get: the current format, RVIO_ERR_INVALID for a NULL handle.
 * The raw formats follow the same rules: stride < width * bytes per pixel is RVIO_ERR_INVALID; a 16-bit format also refuses an odd `stride`,
 * an odd `img_stride` and an odd device address (rvio_hip_last_error says so); a Bayer format on an image narrower or lower than 3 pixels is
 * RVIO_ERR_INVALID here; the staging of the host-buffer entry points grows to width * height * bytes per pixel. */
int rvio_hip_set_image_format(rvio_hip* h, int format);
int rvio_hip_get_image_format(const rvio_hip* h);

/* Copy the device-resident mvFeatTypesForUpdate / mvlFeatMeasForUpdate out.
 * Buffers must hold ceil(n_features/2) entries (x max_track_len x 2 floats). */
int rvio_hip_get_tracks(rvio_hip* h, int32_t* n_feat, unsigned char* types, int32_t* len, float* meas);
/* Tracker's persistent members: mvFeatsToTrack (px) and track lengths. */
int rvio_hip_get_tracker_points(rvio_hip* h, int32_t* n, float* xy, int32_t* hist_len);
/* Updater::update on the tracker's device-resident outputs. */
int rvio_hip_update_tracked(rvio_hip* h);

/* --- whole frame ----------------------------------------------------------- */
/* The timed body of System::MonoVIO (System.cc:253-367): track -> propagate ->
 * [update if nCloneStates > nMinTrackingLength-1] -> augment -> compose, all
 * enqueued on the handle's streams with no host synchronisation; the front end of frame k+1
 * overlaps the filter of frame k.  The call returns before the device has read the inputs:
 * d_img / d_imu / d_cand_xy must stay valid (and unchanged) until the frame has completed on the
 * device, i.e. until rvio_hip_sync or any getter (rvio_hip_get_pose, rvio_hip_get_state, ...)
 * issued after this call has returned.  (rvio_hip_frame, below, has no such condition.) */
int rvio_hip_frame_dev(rvio_hip* h, const uint8_t* d_img, int stride,
                       const rvio_imu* d_imu, int m, const float* d_cand_xy, int n_cand);
/* The same body fed from HOST buffers — what System::MonoVIO holds at System.cc:253-258
 * (pImageData->Image, the IMU list of the frame) plus the detector's corners.  The caller's
 * buffers are packed into a pinned ring on the host and consumed before the call returns; the
 * H2D copies then run asynchronously on the tracker stream (device staging double-buffered by
 * frame parity) and overlap the previous frame's filter work. */
int rvio_hip_frame(rvio_hip* h, const uint8_t* img, int stride,
                   const rvio_imu* imu, int m, const float* cand_xy, int n_cand);
/* The pipelined frame split open for callers that run the update themselves (the feature-sharded
 * updater): frame_begin_dev enqueues PreIntegrator::propagate on the filter stream and the front
 * end on its own streams and orders the filter stream after the front end; the caller then issues
 * rvio_hip_frame_plan, the update (rvio_hip_update_local -> collective on rvio_hip_stream ->
 * rvio_hip_update_global, or rvio_hip_update_tracked) and rvio_hip_augment_compose; frame_end
 * closes the frame.  No host synchronisation anywhere. */
int rvio_hip_frame_begin_dev(rvio_hip* h, const uint8_t* d_img, int stride,
                             const rvio_imu* d_imu, int m, const float* d_cand_xy, int n_cand);
int rvio_hip_frame_end(rvio_hip* h);
/* For callers that sequence the frame themselves (per-stage timing, the sharded updater):
 * frame_plan advances nImageCountAfterInit and reports MonoVIO's two data-independent
 * branches (System.cc:266 `nCloneStates > mnMinCloneStates`, System.cc:280
 * `nImageCountAfterInit > 1`); propagate_dev is rvio_hip_propagate on device-resident IMU. */
int rvio_hip_frame_plan(rvio_hip* h, int* do_update, int* do_augment);
int rvio_hip_propagate_dev(rvio_hip* h, const rvio_imu* d_imu, int m);

/* --- batched instances ---------------------------------- */
/* B independent instances (B robots, each with its own camera: rvio_hip_set_calibration_at below) behind one handle:
 * every buffer of instance i lives in slab i, and every stage is ONE launch with
 * gridDim.z = B, i.e. the single-workgroup stages of one filter become B workgroups.  The
 * arithmetic of an instance is the arithmetic of a plain handle, bit for bit.  The reference
 * runs one System per process (System.cc:38-41 globals); this is the multi-robot form of the
 * same calls.  front_end = 0: the filter only (PreIntegrator::propagate, Updater::update,
 * augmentation/composition; driven by rvio_hip_frame_tracks_dev); front_end = 1: Tracker::track
 * as well (CLAHE, DetectWithSubPix, KLT, RANSAC, book-keeping; driven by
 * rvio_hip_frame_batch_dev).  The single-instance entry points return RVIO_ERR_UNSUPPORTED on
 * a batch handle; the window length is common to all instances (it depends on the frame count
 * only, System.cc:266,280).  rvio_hip_set_state / rvio_hip_initialize give every instance the
 * same state (rvio_hip_set_state_at / rvio_hip_initialize_at: one instance), rvio_hip_get_state reads instance 0.  Every instance starts
 * with the camera calibration of `cfg`; a fleet then binds each robot's own (see "per-instance calibration"). */
int rvio_hip_create_batch(const rvio_config* cfg, int device, int n_instances, int front_end,
                          rvio_hip** out);
int rvio_hip_batch_size(const rvio_hip* h);
int rvio_hip_set_state_at(rvio_hip* h, int instance, const double* x, int xdim, const double* P, int d);
int rvio_hip_get_state_at(rvio_hip* h, int instance, double* x, int* xdim, double* P, int* d);
/* System::initialize (System.cc:115-170) for ONE instance: each robot has its own gravity direction and biases.  The x(26), P(24 x 24) that
 * rvio_hip_initialize computes from (w, a, n_imu), stored as rvio_hip_set_state_at stores them — and none of the handle-wide resets of
 * rvio_hip_initialize (frame count, tracker, landmark cloud, odometry ring), so it belongs between create / rvio_hip_initialize and the
 * first frame: RVIO_ERR_STATE when the window is not empty, RVIO_ERR_INVALID for a NULL argument or an instance out of range. */
int rvio_hip_initialize_at(rvio_hip* h, int instance, const double w[3], const double a[3], int n_imu);

/* --- per-instance calibration ---------------------------------------------------- */
/* What differs between two physical cameras: the intrinsics, the distortion model and the camera-IMU extrinsic.  A handle is created with
 * one rvio_config, and every instance starts with that config's calibration; these entry points give instance i its own, so that a batch
 * handle serves B different robots.  The calibration is read by the undistortion (Tracker.cc:100-130) and RANSAC's gyro prior
 * (Ransac.cc:120-155) in the front end, and by the per-feature triangulation / Jacobian stage (Updater.cc:114-375) and the landmark cloud
 * (Updater.cc:430-448) in the filter: the arithmetic of an instance is that of a handle created with its calibration in the config, bit for
 * bit.
 * DELIBERATELY HANDLE-WIDE (common to all instances, taken from the config at create): the image size (width, height); sigma_px / sigma_py
 * (the measurement noise sigma_im); every Tracker.* key (n_features, max_track_len, min_track_len, min_dist, qual_lvl, block_x, block_y,
 * enable_equalizer, use_sampson, inlier_thr); every IMU.* key (imu_rate, the four sigmas, gravity, small_angle); every INI.* key. */
typedef struct rvio_calibration {   /* 168 bytes, no padding */
    float fx, fy, cx, cy;           /* Tracker.cc:39-42 */
    float k1, k2, p1, p2, k3;       /* Tracker.cc:51-61 */
    int32_t fisheye;                /* Camera.Fisheye */
    double T_bc[16];                /* Camera.T_BC0, ROW-major 4x4, rows 0..2 are read (Updater.cc:46-53) */
} rvio_calibration;
/* the calibration members of a config, copied */
void rvio_calibration_from_config(const rvio_config* cfg, rvio_calibration* out);
/* set: one instance / all of them (`all` holds rvio_hip_batch_size entries, uploaded in one copy).  A setter drains the handle, as
 * rvio_hip_set_image_format does, and holds from the next call enqueued.  The first setter allocates a table of one entry per instance
 * outside the filter slab (filled from the config); a handle on which none was ever called allocates nothing and launches what it launched
 * before these entry points existed.  A plain handle is accepted with instance 0 only: re-calibration without re-creating the handle, also for
 * the ranks of the feature-sharded updater (set every rank alike).
 * Meant to be called BEFORE THE FIRST FRAME: observations already in a tracking history keep the normalised coordinates they were recorded
 * with (they were undistorted under the calibration of their frame), so a change in mid-sequence mixes the two until those tracks have ended.
 * rvio_hip_initialize, rvio_hip_set_state and rvio_hip_set_state_at leave calibrations alone, and so does rvio_hip_debug_poison.
 * RVIO_ERR_INVALID: NULL handle or calibration, instance out of range, a non-finite member (any of the nine floats or sixteen doubles), fx or
 * fy equal to 0 (rvio_hip_last_error names the instance).
 * get: what instance i computes with — the config's values until a setter changed them. */
int rvio_hip_set_calibration_at(rvio_hip* h, int instance, const rvio_calibration* cal);
int rvio_hip_set_calibrations(rvio_hip* h, const rvio_calibration* all /* rvio_hip_batch_size entries, one copy */);
int rvio_hip_get_calibration_at(rvio_hip* h, int instance, rvio_calibration* cal);

/* rvio_hip_get_tracker_points of one instance (batch handle with front end): Tracker::mvFeatsToTrack
 * and the length of each feature's tracking history. */
int rvio_hip_get_tracker_points_at(rvio_hip* h, int instance, int32_t* n, float* xy, int32_t* hist_len);
/* The body of System::MonoVIO after Tracker::track (System.cc:263-365: propagate, update if
 * nCloneStates > mnMinCloneStates, augmentation + composition) on DEVICE-resident hand-over
 * tables, for all B instances of the handle (B = 1 for a plain handle):
 *   d_n_feat[B], d_types[B][Fu], d_len[B][Fu], d_meas[B][Fu][max_track_len][2]
 * (Tracker::mvFeatTypesForUpdate / mvlFeatMeasForUpdate, Tracker.h:67-74, Fu = ceil(nFeatures/2));
 * d_imu[B][imu_stride] samples, imu_stride = 0: one IMU batch shared by all instances.
 * Track lengths must satisfy 2 <= len <= window length + 1 (what Tracker::track emits). */
int rvio_hip_frame_tracks_dev(rvio_hip* h, const rvio_imu* d_imu, int imu_stride, int m,
                              const int32_t* d_n_feat, const unsigned char* d_types,
                              const int32_t* d_len, const float* d_meas);
/* One camera frame of every instance (the whole timed body of System::MonoVIO, System.cc:253-367,
 * pipelined like rvio_hip_frame_dev): d_imgs = B mono8 images, `img_stride` bytes apart, rows
 * `stride` bytes apart; d_imu[B][imu_stride] (0: shared).  Corners come from the device detector. */
int rvio_hip_frame_batch_dev(rvio_hip* h, const uint8_t* d_imgs, int stride, size_t img_stride,
                             const rvio_imu* d_imu, int imu_stride, int m);
/* same, direct-track mode, host inputs */
int rvio_hip_frame_points(rvio_hip* h, const float* tracked_xy, const unsigned char* status, int n_pts,
                          const rvio_imu* imu, int m, const float* cand_xy, int n_cand);
int rvio_hip_get_frame_info(rvio_hip* h, rvio_frame_info* info);
/* pose line of stamped_pose_ests.dat (System.cc:371-374): pGk(3), qkG(4) */
int rvio_hip_get_pose(rvio_hip* h, double p[3], double q[4]);
/* the same line of one instance of a batch handle (RVIO_ERR_INVALID out of range); on a plain handle instance 0 is rvio_hip_get_pose */
int rvio_hip_get_pose_at(rvio_hip* h, int instance, double p[3], double q[4]);

/* --- odometry ring ----------------------------------------------------------- */
/* What System::MonoVIO publishes every frame — nav_msgs::Odometry (System.cc:402-418: the pose, twist.linear = vk) and the pose appended to
 * nav_msgs::Path (System.cc:420-434) — kept on the device: one record per instance and frame, written by a kernel of its own behind the
 * augmentation / composition stage of EVERY path (stage by stage, rvio_hip_frame*, rvio_hip_frame_points, the sharded frame, batch handles),
 * into a ring that is read back in bulk.  A host that wants every pose no longer drains the pipeline once per frame. */
typedef struct rvio_odom {          /* 464 bytes, no padding */
    int64_t seq;        /* 1, 2, ...: augment/compose stages of this handle recorded since create / rvio_hip_initialize (stages run while the ring is off are not counted) */
    int32_t img_count;  /* nImageCountAfterInit of that frame (System.cc:251) */
    int32_t n_clones;   /* nCloneStates after the frame */
    int32_t reserved[2];/* 0 */
    double p[3];        /* pGk, System.cc:341  -- the bits rvio_hip_get_pose returns */
    double q[4];        /* qkG, System.cc:339  -- the same */
    double v[3];        /* vk,  System.cc:331,414-416 = x[17..19] behind the frame */
    double pose_cov[36];/* row-major 6x6, order (x, y, z, rot X, rot Y, rot Z): nav_msgs/Odometry pose.covariance (the reference leaves it at zero).
                         * With R = R(qkG), p = pkG = x[4..6] and P6 = P[0..5][0..5] behind the frame — the error (dth, dp) of the reference's
                         * injection (Updater.cc:549-566), R_true ~ (I - [dth x]) R — and the published pGk = -R^T p, R_wb = R^T, world-frame rotation
                         * error phi (R_wb,true ~ (I + [phi x]) R_wb):  J = [ R^T [p x], -R^T ; R^T, 0 ],  pose_cov = (C + C^T) / 2, C = J P6 J^T.
                         * Exactly symmetric. */
    double vel_cov[9];  /* row-major P[15..17][15..17] behind the frame, copied */
} rvio_odom;
/* capacity = records kept per instance: 0 = off (the default: such a handle allocates and launches what it did before these entry points
 * existed), 1 .. 65536.  The first enable drains the handle and allocates the ring, outside the filter slab, laid out
 * ring[(seq - 1) % capacity][instance] (one frame's records of all instances are contiguous); another capacity drains, reallocates and
 * empties the ring (seq restarts at 1); 0 stops the launches and keeps the ring and its records; the same capacity again resumes.
 * rvio_hip_initialize empties the ring, rvio_hip_set_state leaves it alone.  RVIO_ERR_INVALID: NULL handle, capacity outside 0 .. 65536;
 * RVIO_ERR_UNSUPPORTED (rvio_hip_last_error names the size): capacity x instances x 464 bytes exceeds 1 GiB. */
int rvio_hip_set_odometry(rvio_hip* h, int capacity);
/* The records of one instance with seq in [max(first_seq, newest - capacity + 1, 1), newest], oldest first, at most max_n; *n = how many
 * (0 with RVIO_OK when none qualifies).  `newest` is counted on the host: nothing is read from the device to learn it.  Waits for the
 * filter stream only, like rvio_hip_get_pose.  RVIO_ERR_STATE: the ring was never enabled; RVIO_ERR_INVALID: instance out of range,
 * max_n < 0, out == NULL with max_n > 0. */
int rvio_hip_get_odometry(rvio_hip* h, int instance, int64_t first_seq, int max_n, rvio_odom* out, int32_t* n);
/* The newest record of every instance in one copy: out holds rvio_hip_batch_size records, *seq their seq (0 before the first frame: nothing
 * is copied).  Where all robots of a fleet are, per frame, without one state read-back per instance. */
int rvio_hip_get_odometry_all(rvio_hip* h, rvio_odom* out /* batch records */, int64_t* seq);

/* --- IMU-rate odometry ------------------------------------------------------- */
/* A pose at every IMU sample.  PreIntegrator::propagate has (Rk, pk, vk) complete at the bottom of every iteration of its sample loop
 * (PreIntegrator.cc:168-176) and keeps only the last; a kernel of its own (csrc/imu_pose.hip) runs the same loop on the states alone — no
 * Phi, no Q, no covariance — and keeps them all.  Record j is the pose line System::MonoVIO would write if an image arrived right behind
 * sample j and that frame ran no update; both branches of nSmallAngle are carried.  The loop starts from x[0..25] = qG, pG, g, qk, pk, v,
 * bg, ba as they are, a non-identity qk included (Rk starts at QuatToRot(qk); pk is rebuilt from v, g, Dt and dp, as upstream).
 * Two uses: dead reckoning between two images (rvio_hip_predict*: no side effect on the filter) and a dense trajectory (the ring). */
typedef struct rvio_imu_pose {   /* 104 bytes, no padding */
    int64_t seq;        /* ring records: 1, 2, ... IMU samples of this handle recorded since create / rvio_hip_initialize; rvio_hip_predict*: 0 */
    int32_t img_count;  /* nImageCountAfterInit of the frame whose propagate consumes the sample (predict: the handle's current count) */
    int32_t index;      /* j: position of the sample in its batch */
    double t;           /* imu[j].t, copied */
    double p[3];        /* pGj = R(qG)^T (pk_j - pG)                   (System.cc:341 with pk_j for pk) */
    double q[4];        /* qjG = QuatMul(RotToQuat(Rk_j), qG), JPL xyzw (System.cc:339, PreIntegrator.cc:182) */
    double v[3];        /* vk_j                                        (PreIntegrator.cc:176; what twist.linear carries, System.cc:414-416) */
} rvio_imu_pose;
/* Dead reckoning: the records of imu[0 .. m) from the CURRENT state of one instance.  Mutates nothing — not x, P, the frame count, the tracker
 * or either ring.  Host buffers in and out, staged through device buffers of the call's own (allocated by the first call, outside the
 * filter slab; m > RVIO_HIP_MAX_IMU grows them); waits for the filter stream like rvio_hip_get_pose, so the state is the one behind every
 * frame enqueued so far.  m == 0: RVIO_OK, nothing written.  RVIO_ERR_INVALID: NULL handle, instance out of range, m < 0, a NULL buffer with
 * m > 0; RVIO_ERR_STATE: before the first rvio_hip_set_state / rvio_hip_initialize. */
int rvio_hip_predict(rvio_hip* h, int instance, const rvio_imu* imu, int m, rvio_imu_pose* out);
/* The same for EVERY instance in one launch, device buffers, asynchronous on rvio_hip_stream (it reads the state behind everything already
 * enqueued there): d_out[z * out_stride + j] for instance z, out_stride >= m records; d_imu[z * imu_stride + j], imu_stride = 0: one batch
 * shared by all instances, else >= m (the rules of rvio_hip_frame_tracks_dev).  Violations: RVIO_ERR_INVALID. */
int rvio_hip_predict_dev(rvio_hip* h, const rvio_imu* d_imu, int imu_stride, int m, rvio_imu_pose* d_out, int out_stride);
/* The IMU-rate ring: every IMU sample that ANY propagate of this handle consumes leaves a record (stage by stage, rvio_hip_frame*,
 * rvio_hip_frame_points, rvio_hip_frame_begin_dev, the sharded frame — every rank alike —, both batch frames), written by the same kernel
 * directly in front of the launch that propagates in place, on that launch's stream.  img_count is the count of the frame the samples
 * belong to; a caller that sequences the stages itself calls rvio_hip_frame_plan ahead of rvio_hip_propagate*, as System::MonoVIO's order
 * has it.  capacity = samples kept per instance: 0 = off (the default: such a handle allocates and launches what it did before these entry
 * points existed), 1 .. 1048576.  The first enable drains the handle and allocates the ring, outside the filter slab, laid out
 * ring[(seq - 1) % capacity][instance]; another capacity drains, reallocates and empties the ring (seq restarts at 1); 0 stops the launches
 * and keeps the ring and its records; the same capacity again resumes.  Of a batch longer than the capacity the last `capacity` records
 * survive.  rvio_hip_initialize empties the ring; rvio_hip_set_state* and rvio_hip_debug_poison leave it alone.  RVIO_ERR_INVALID: NULL
 * handle, capacity outside 0 .. 1048576; RVIO_ERR_UNSUPPORTED (rvio_hip_last_error names the size): capacity x instances x 104 bytes
 * exceeds 1 GiB. */
int rvio_hip_set_imu_odometry(rvio_hip* h, int capacity);
/* rvio_hip_get_odometry's semantics on that ring: the records of one instance with seq in [max(first_seq, newest - capacity + 1, 1), newest],
 * oldest first, at most max_n; *n = how many.  `newest` is counted on the host from the m of each call.  Waits for the filter stream only.
 * RVIO_ERR_STATE: the ring was never enabled; RVIO_ERR_INVALID: instance out of range, max_n < 0, out == NULL with max_n > 0. */
int rvio_hip_get_imu_odometry(rvio_hip* h, int instance, int64_t first_seq, int max_n, rvio_imu_pose* out, int32_t* n);

/* --- IMU-rate odometry with covariance (added within ABI 6) ------------------- */
/* The pose_cov / vel_cov an rvio_odom record would carry for the hypothetical frame behind record j of IMU-rate odometry ("an image arrives
 * right behind sample j and that frame runs no update"), for every sample, by a kernel of its own (csrc/imu_cov.hip); the pose records
 * stay imu_pose_kernel's.
 *   1  P11_0 = P[0..23][0..23] of the current covariance.
 *   2  per sample s: P11 <- Phi_s P11 Phi_s^T + Q_s, Phi_s = I + dt F_s, Q_s = (dt G_s) Sigma G_s^T (PreIntegrator.cc:123-142), F_s and G_s built
 *      from Rk, Rk^T, vk, gk as they stand IN FRONT of step s — behind step s - 1; at s = 0 QuatToRot(x[10..13]), x[17..19] and the raw
 *      x[7..9]; gk is re-normalised Rk gR behind every step.  No clone cross-terms: the marginal of the head does not depend on them.
 *   3  behind step j: P6_j = Vk_j[0..5][:] P11_j Vk_j[0..5][:]^T, Vk_j composition's Jacobian (System.cc:325-365) from (Rk_j, pk_j, pG); its
 *      top six rows touch columns 0-5 and 9-14 only.
 *   4  pose_cov_j = (C + C^T) / 2, C = J_j P6_j J_j^T, J_j the 6 x 6 map of rvio_odom.pose_cov at the composed (qjG, pjG = Rk_j (pG - pk_j));
 *      order (x, y, z, rot X, rot Y, rot Z), exactly symmetric.
 *   5  vel_cov_j = sym(P11_j)[15..17][15..17] (Vk is the identity there), exactly symmetric. */
typedef struct rvio_imu_cov {   /* 376 bytes, no padding */
    int64_t seq;        /* the paired rvio_imu_pose's */
    int32_t img_count;  /* the paired rvio_imu_pose's */
    int32_t index;      /* the paired rvio_imu_pose's */
    double pose_cov[36];   /* row-major 6 x 6 */
    double vel_cov[9];     /* row-major 3 x 3, of vk_j (IMU frame) */
} rvio_imu_cov;
/* rvio_hip_predict's contract plus the covariance records: no side effect on x, P, the frame count, the tracker or any ring; the pose records
 * are the existing kernel's and out may be NULL (covariances only); m > RVIO_HIP_MAX_IMU grows the staging.  Errors: rvio_hip_predict's, with
 * cov in place of out as the buffer that must not be NULL. */
int rvio_hip_predict_cov(rvio_hip* h, int instance, const rvio_imu* imu, int m, rvio_imu_pose* out, rvio_imu_cov* cov);
/* rvio_hip_predict_dev's contract plus d_cov[z * cov_stride + j], cov_stride >= m; d_out may be NULL (out_stride is then ignored). */
int rvio_hip_predict_cov_dev(rvio_hip* h, const rvio_imu* d_imu, int imu_stride, int m, rvio_imu_pose* d_out, int out_stride, rvio_imu_cov* d_cov, int cov_stride);
/* A second ring, paired with the IMU-rate ring: its capacity, its seq, its slot rule ring[(seq - 1) % capacity][instance].  enable = 1: from
 * now on imu_cov_kernel runs right next to imu_pose_kernel — in front of every launch that propagates in place, on that launch's stream, on
 * every path the pose ring covers (while the pose ring records: its capacity 0 stops both).  The first enable drains the handle and allocates
 * the ring outside the filter slab.  enable = 0 stops the launches and keeps the records.  A capacity change through
 * rvio_hip_set_imu_odometry reallocates and empties both rings, rvio_hip_initialize empties both.  Default off: a handle that never enables
 * it allocates and launches what it did before.  RVIO_ERR_INVALID: NULL handle, enable outside 0 / 1; RVIO_ERR_STATE: enable = 1 and the
 * IMU-rate ring was never enabled; RVIO_ERR_UNSUPPORTED (rvio_hip_last_error names the size): capacity x instances x 376 bytes exceeds 1 GiB
 * (also returned by rvio_hip_set_imu_odometry when a capacity change would take an existing covariance ring beyond that: nothing changes). */
int rvio_hip_set_imu_odometry_cov(rvio_hip* h, int enable);
/* rvio_hip_get_imu_odometry's window rule on that ring, restricted to the records with seq >= the first sample recorded since covariance was
 * last switched on.  Bounds are counted on the host; waits for the filter stream only.  RVIO_ERR_STATE: the covariance ring was never
 * enabled; RVIO_ERR_INVALID: instance out of range, max_n < 0, out == NULL with max_n > 0. */
int rvio_hip_get_imu_odometry_cov(rvio_hip* h, int instance, int64_t first_seq, int max_n, rvio_imu_cov* out, int32_t* n);

/* --- auxiliary measurement update (no reference counterpart) ----------------- */
/* Fuses what is not a camera track — wheel odometry, a zero-velocity update, a speed-over-ground sensor — on the device: at most
 * RVIO_AUX_MAX_ROWS rows of a measurement the caller has linearised, z = h(x) + noise, with a FULL-WIDTH Jacobian.  The arithmetic of
 * Updater.cc:540-619 on the whitened rows H~ = H / sigma, v~ = v / sigma (row-wise; R = diag(sigma^2) becomes I):
 *   S = H~ P H~^T + I,   K = P H~^T S^-1,   dx = K v~,   gamma = v~^T S^-1 v~,   P <- (I - K H~) P (I - K H~)^T + K K^T   (Joseph form)
 * H: m x d ROW-major, d = 24 + 6 n for the window as it is NOW (rvio_hip_get_state's d).  Its columns are the ERROR-state coordinates in the
 * order of P: 0-2 rotation of qG, 3-5 pG, 6-8 g, 9-11 rotation of qk, 12-14 pk, 15-17 v (IMU frame), 18-20 bg, 21-23 ba, then per clone p
 * (oldest first) 24+6p .. 26+6p rotation, 27+6p .. 29+6p position.  State injection is Updater.cc:546-613: q <- QuatMul([dth / 2; sqrt(1 -
 * |dth / 2|^2)], q) in the three kinds of rotation slots, g re-normalised behind its addition, everything else x <- x + dx.  (An all-zero qk — what
 * System::initialize leaves until the first composition, read as I by QuatToRot — is injected as the identity it stands for.)  P stays
 * symmetric bit for bit.
 * mode: RVIO_AUX_RESIDUAL: v is the residual r = z - h(x), formed by the caller.  RVIO_AUX_VALUE: v is the measured value z of a LINEAR
 *   measurement of the additive coordinates and the device forms r = z - H xi(x), where xi(x) is x in error-state order with 0 in every rotation
 *   slot: xi[3..8] = x[4..9], xi[12..23] = x[14..25], xi[27+6p .. 29+6p] = x[30+7p .. 32+7p].  Zero velocity: m = 3, H = I at columns 15..17,
 *   z = 0; a velocity in the IMU frame: the same with z = v_meas.  No state is read back to form a residual.
 *   (Measurements that are NOT linear in these coordinates — a world-frame position, attitude or pose, the accelerometer at rest — are
 *   linearised on the device by rvio_hip_update_fix below.)
 * gate: 0: always apply; 1: apply iff |gamma| < chi2inv(0.95, m), the table and the comparison of the feature gate (Updater.cc:422).
 * In place: x and P of the current buffer are updated where they lie (no double-buffer toggle); an instance that is gated out, inactive or
 * indefinite is not written at all.  The pose line (rvio_hip_get_pose[_at]) is rewritten from the updated state, (pGk, qkG) =
 * (R(qG)^T (pk - pG), QuatMul(qk, qG)); NO record is appended to the odometry ring or the IMU-rate ring: those stay one record per frame /
 * per IMU sample.  A clone-block factor kept for the next visual update is dropped (that update factors the new covariance itself).
 * When: whenever the handle has a state — behind rvio_hip_initialize with an empty window (d = 24), between two whole frames, between the
 * stage entry points.  RVIO_ERR_STATE: no state yet, or between rvio_hip_frame_begin_dev and rvio_hip_frame_end.
 * Handle-wide: the window length (hence d) and m, mode, gate of a call; per instance: H, v, sigma (by stride) and whether the call applies.
 * Plain, batch (with or without front end) and sharded handles alike; a sharded rank holds a replica of the state: call it on every rank
 * alike, as the calibration setters.  A handle that never calls these allocates and launches what it did before they existed.
 * A non-positive pivot of S (the covariance handed in was indefinite) sets the sticky device error bit 8 (rvio_frame_info.reserved[0]) and
 * leaves that instance untouched, applied = 0 — what the feature gate does. */
#define RVIO_AUX_MAX_ROWS 16
typedef enum { RVIO_AUX_RESIDUAL = 0, RVIO_AUX_VALUE = 1 } rvio_aux_mode;
typedef struct rvio_aux_meas {   /* 40 bytes; host pointers */
    int32_t m;            /* rows, 1 .. RVIO_AUX_MAX_ROWS */
    int32_t mode;         /* rvio_aux_mode */
    int32_t gate;         /* 0 | 1 */
    int32_t reserved;
    const double* H;      /* m x d row-major */
    const double* v;      /* m: r (RESIDUAL) or z (VALUE) */
    const double* sigma;  /* m standard deviations, finite and > 0 */
} rvio_aux_meas;
/* Host buffers: checked, staged through a pinned block of the call's own (allocated by the first call, outside the filter slab) and
 * enqueued on the filter stream; the call does not wait for that stream.  instance: 0 .. B - 1, or -1: every instance, the same measurement.
 * RVIO_ERR_INVALID: a NULL argument, m or instance out of range, an unknown mode, gate not 0 | 1, a non-finite value in H, v or sigma, a
 * sigma <= 0, or — VALUE mode — a non-zero entry in a rotation column of H (xi is 0 there, so the residual would silently ignore it). */
int rvio_hip_update_aux(rvio_hip* h, int instance, const rvio_aux_meas* meas);
/* Device buffers, EVERY instance in one launch, asynchronous on rvio_hip_stream with no host synchronisation: instance z reads
 * d_H + z * H_stride, d_v + z * v_stride, d_sigma + z * sigma_stride (strides in doubles; 0: one array shared by all instances, else
 * H_stride >= m d and the others >= m).  d_active: NULL = all instances, else B flags, 0 = leave that instance untouched (applied = 0).
 * Values are NOT checked: finite entries, sigma > 0 and — VALUE mode — zero rotation columns of H are the caller's responsibility.
 * RVIO_ERR_INVALID: a NULL handle, d_H, d_v or d_sigma, m outside 1 .. RVIO_AUX_MAX_ROWS, an unknown mode, gate not 0 | 1, a stride too short. */
int rvio_hip_update_aux_dev(rvio_hip* h, int m, int mode, int gate, const double* d_H, size_t H_stride, const double* d_v, size_t v_stride,
                            const double* d_sigma, size_t sigma_stride, const int32_t* d_active);
/* gamma (as compared: |v~^T S^-1 v~|) and applied (1 applied; 0 gated out, inactive or a bad pivot) of one instance in the LAST call.  Waits
 * for the filter stream only.  RVIO_ERR_STATE before the first rvio_hip_update_aux* call; RVIO_ERR_INVALID: instance out of range. */
int rvio_hip_get_aux_diag(rvio_hip* h, int instance, double* gamma, int32_t* applied);

/* --- standstill detection and automatic zero-velocity update (no reference counterpart during operation; System.cc:185-250 tests only
 *     in front of initialisation) ------------------------------------------------ */
/* Decides ON THE DEVICE, per instance, whether the platform stands still, and — with apply = 1 — hands that decision to the auxiliary update
 * above as its d_active flags: a zero-velocity update (and optionally a gyro-bias update) of exactly the instances that are static, without the
 * host seeing the biases, the tracker's points or the decision.  One launch of standstill_kernel (csrc/standstill.hip), one workgroup per
 * instance, then aux_update_kernel right behind it.
 * IMU statistic (SHOE / GLRT, Skog et al. 2010; no attitude in it): with bg = x[20..22], ba = x[23..25] of the instance's current state,
 * G = cfg.gravity and the m samples handed in,
 *     a^_j = a_j - ba,  w^_j = w_j - bg,  a_ = mean(a^_j),  u = a_ / |a_|
 *     T = (1/m) sum_j ( |a^_j - G u|^2 / sigma_a^2 + |w^_j|^2 / sigma_w^2 ),     imu_static = (T < imu_thr)
 *   (|a_| = 0 or a non-finite T: not static).
 * Image statistic (handles with a front end): over the live points with at least two observations, the mean length in PIXELS of the step
 *   between the last two observations of the tracking history, (fx dx, fy dy) with the instance's calibration.  It can only veto:
 *     img_static = (disp_thr_px <= 0) || (n_pairs < min_pairs) || (disparity < disp_thr_px)
 *   A handle without front end reports n_pairs = 0, disparity = 0, img_static = 1.
 * is_static = imu_static && img_static.
 * The update (apply = 1): RVIO_AUX_VALUE, rows 0..2: H = I at the velocity columns 15..17, z = 0, sigma_v; with bias_rows = 1 three more rows,
 *   H = I at the gyro-bias columns 18..20, z = the mean RAW gyro reading of the batch (at rest w_m = bg + noise), sigma_bg.  Everything
 *   rvio_hip_update_aux_dev documents holds: in place, pose line rewritten, no ring record, a kept clone-block factor dropped, an instance that
 *   is not static (or gated out) not written at all.
 * The defaults of rvio_standstill_config_default are TUNING VALUES, not measurements: sigma_a / sigma_w are the discrete-time form of the
 *   configured densities (cfg.sigma_a sqrt(imu_rate), cfg.sigma_g sqrt(imu_rate)), under which T has mean ~ 6, imu_thr = 12 is twice that;
 *   disp_thr_px = 0.5, min_pairs = 20, sigma_v = 0.05, sigma_bg = sigma_w, bias_rows = 0, gate = 1.
 * NOT done: a static frame still runs its camera update and augments a clone (skipping both would change the frame path); the accelerometer
 *   rows a_m = ba + G R_k g are not fused BY THIS CALL.  They exist as RVIO_FIX_GRAVITY (rvio_hip_update_fix below, linearised on the device): a
 *   caller applies them when rvio_hip_get_standstill says static, or hands rvio_hip_update_fix_dev its own flags. */
typedef struct rvio_standstill_config {   /* 64 bytes, no padding */
    double sigma_a, sigma_w;      /* detector noise, m/s^2 and rad/s per sample, finite and > 0 */
    double imu_thr;               /* > 0 */
    double disp_thr_px;           /* <= 0: image test off */
    double sigma_v, sigma_bg;     /* the update's standard deviations, finite and > 0 */
    int32_t min_pairs;            /* >= 1 */
    int32_t bias_rows;            /* 0 | 1 */
    int32_t gate;                 /* 0 | 1: the aux update's chi-square gate */
    int32_t reserved;
} rvio_standstill_config;
typedef struct rvio_standstill {          /* 40 bytes, no padding */
    double T;            /* the IMU statistic, as computed */
    double disparity;    /* px, 0 with n_pairs == 0 */
    double gamma;        /* the aux update's, 0 when not applied */
    int32_t n_pairs;
    int32_t flags;       /* bit 0 imu_static, 1 img_static, 2 is_static, 3 applied */
    int32_t m;           /* samples looked at */
    int32_t img_count;   /* the handle's frame count at the call */
} rvio_standstill;
void rvio_standstill_config_default(const rvio_config* cfg, rvio_standstill_config* out);
/* Switches the feature on with *c (copied), or off with NULL.  Nothing is allocated before the first rvio_hip_standstill* call (then: records,
 * flags, v, H at 6 x d_max, sigma — outside the filter slab); a handle that never calls this allocates and launches what it did before.
 * RVIO_ERR_INVALID: NULL handle or a bad member — rvio_hip_last_error names it. */
int rvio_hip_set_standstill(rvio_hip* h, const rvio_standstill_config* c);
/* One decision per instance from m IMU samples (host buffer: every instance sees the same batch; _dev: device buffer, instance z reads
 * d_imu + z * imu_stride, imu_stride = 0: shared, else >= m — the rules of rvio_hip_predict_dev).  apply: 0 = detect only: nothing but the
 * standstill records changes; 1 = the update above on the static instances.  Asynchronous on rvio_hip_stream, no host wait: the detector is
 * ordered behind the book-keeping of the last frame and in front of the next one's by stream events (it runs on the stream that runs
 * book-keeping; the filter stream waits for it in front of the update).  Call it between whole frames or between the stage entry points, on
 * every rank of a sharded handle alike.  RVIO_ERR_STATE: no state yet, rvio_hip_set_standstill not called (or called with NULL), between
 * rvio_hip_frame_begin_dev and rvio_hip_frame_end.  RVIO_ERR_INVALID: NULL handle or buffer, m < 1, apply not 0 | 1, a stride too short. */
int rvio_hip_standstill(rvio_hip* h, const rvio_imu* imu, int m, int apply);
int rvio_hip_standstill_dev(rvio_hip* h, const rvio_imu* d_imu, int imu_stride, int m, int apply);
/* The record of one instance from the LAST rvio_hip_standstill* call; waits for the filter stream only.  RVIO_ERR_STATE before the first such
 * call; RVIO_ERR_INVALID: NULL argument, instance out of range. */
int rvio_hip_get_standstill(rvio_hip* h, int instance, rvio_standstill* out);

/* --- absolute fixes: world-frame position, attitude, pose; the accelerometer at rest (no reference counterpart) ------------------ */
/* rvio_hip_update_aux fuses what the caller has linearised; these measurements are not linear in the robocentric state, and linearising them
 * on the host costs a drain and a state read-back per fix.  Here the linearisation happens where the state is: fix_rows_kernel
 * (csrc/fix_rows.hip, one wave per instance) writes (H, r, sigma) at the instance's CURRENT state and aux_update_kernel, unchanged, runs right
 * behind it in RVIO_AUX_RESIDUAL mode with m = 3 (POSE: 6) rows.
 * Frames and conventions are those of rvio_hip_get_pose: a position is pGk = R(qG)^T (pk - pG), a quaternion is qkG = QuatMul(qk, qG), JPL xyzw,
 * rotating world vectors into the IMU frame.  THE FILTER'S WORLD FRAME IS THE FIRST IMU FRAME AND IS NOT GRAVITY-ALIGNED — hence no heading-only
 * kind; aligning an ENU or motion-capture frame to it, and re-expressing a sensor's attitude as the IMU's, is the caller's job.
 * With R_G = R(x[0:4]), R_k = R(x[10:14]) (an all-zero qk reads as I), R = R_k R_G, l = lever, s = pk - pG + R_k^T l, G = cfg.gravity, g = x[7:10],
 * the columns of P as rvio_hip_update_aux documents them and R_true ~ (I - [dth x]) R in every rotation slot (all columns not listed are 0):
 *   POSITION  m = 3  h = R_G^T s                     r = z[0:3] - h
 *                    cols 0-2: -R_G^T [s x]   3-5: -R_G^T   9-11: -R_G^T R_k^T [l x]   12-14: R_G^T
 *   ATTITUDE  m = 3  the world-frame rotation error phi of R_wb = R^T;  with E = R(z[3:7])^T R:  r = (E21 - E12, E02 - E20, E10 - E01) / 2
 *                    cols 0-2: R_G^T   9-11: R^T
 *   POSE      m = 6  the three position rows, then the three attitude rows
 *   GRAVITY   m = 3  h = ba + G R_k g (PreIntegrator.cc:107, 175-177 at rest)   r = z[0:3] - h,  z[0:3] = the mean RAW accelerometer reading
 *                    cols 6-8: G R_k   9-11: G [R_k g x]   21-23: I
 *             (the state carries g as three coordinates and injection re-normalises it, Updater.cc:566-568: what the gain moves ALONG g is
 *             dropped there, so the part of a residual along gravity is only taken up as far as the prior hands it to ba)
 * The fix is fused at the state the call finds, not at a time stamp of its own: bridging the gap to the sensor's stamp is the caller's.  One
 * update, linearised once (more passes: rvio_hip_set_meas_iterations below).  Everything rvio_hip_update_aux_dev documents holds: in place, `gate` as there, the pose line rewritten, no ring record, a
 * kept clone-block factor dropped, an inactive or gated-out instance not written at all, error bit 8 on a non-positive pivot. */
typedef enum { RVIO_FIX_POSITION = 0, RVIO_FIX_ATTITUDE = 1, RVIO_FIX_POSE = 2, RVIO_FIX_GRAVITY = 3 } rvio_fix_kind;
typedef struct rvio_fix {      /* 128 bytes, no padding */
    double z[7];      /* [0..2] position (POSITION, POSE) or mean raw accelerometer reading (GRAVITY); [3..6] quaternion (ATTITUDE, POSE) */
    double sigma[6];  /* [0..2] go with z[0..2], [3..5] (rad) with the quaternion */
    double lever[3];  /* position of the sensed point in the IMU frame; POSITION and POSE only */
} rvio_fix;
typedef struct rvio_fix_diag { /* 72 bytes, no padding */
    double r[6];         /* the residual as formed on the device, rows m .. 5 are 0 */
    double gamma;        /* the aux update's |r~^T S^-1 r~| as compared with the gate's table, also when the gate refused it; 0: inactive */
    int32_t applied;     /* 1: fused; 0: inactive, gated out or a bad pivot */
    int32_t kind, m;
    int32_t img_count;   /* the handle's frame count at the call */
} rvio_fix_diag;
/* Host record: *fix is checked, staged in a pinned block of the handle's own and consumed on rvio_hip_stream — no wait for the stream.  instance:
 * 0 .. batch - 1, or -1: every instance gets the same fix.  _dev: device records, instance z reads d_fix + z * fix_stride RECORDS (0: shared);
 * d_active: NULL or one int32 per instance, 0 = leave this instance alone; the values are not checked, as in rvio_hip_update_aux_dev.  kind and
 * gate hold for the whole call.  The first call allocates the feature's block outside the filter slab (the rows at 6 x d_max per instance, r,
 * sigma, the records, the (gamma, applied) pairs of ITS aux launches — a later rvio_hip_update_aux does not overwrite them — and the staging of
 * the host form); a handle that never calls these allocates and launches what it did before.  Plain, batch and sharded handles; on a sharded
 * handle every rank calls alike.
 * RVIO_ERR_STATE: no state yet, between rvio_hip_frame_begin_dev and rvio_hip_frame_end.  RVIO_ERR_INVALID: NULL handle or record, kind, gate or
 * instance out of range and — host form only — a non-finite entry the kind uses, a used sigma <= 0, | |q| - 1 | > 1e-6 (rvio_hip_last_error). */
int rvio_hip_update_fix(rvio_hip* h, int instance, int kind, int gate, const rvio_fix* fix);
int rvio_hip_update_fix_dev(rvio_hip* h, int kind, int gate, const rvio_fix* d_fix, size_t fix_stride, const int32_t* d_active);
/* The record of one instance from the LAST rvio_hip_update_fix* call (an instance that call left alone keeps r of the call that last touched
 * it, with applied = 0); waits for the filter stream only.  RVIO_ERR_STATE before the first such call; RVIO_ERR_INVALID: NULL argument, instance
 * out of range. */
int rvio_hip_get_fix(rvio_hip* h, int instance, rvio_fix_diag* out);
/* The rows the device formed in that call: *m, *d (= 24 + 6 clones at the call), H (m x d row-major) and sigma (m); H and sigma may be NULL —
 * ask for m and d first.  Handing them with the record's r to rvio_hip_update_aux (RVIO_AUX_RESIDUAL) at the same state repeats the update bit
 * for bit.  Waits for the filter stream only.  Errors as rvio_hip_get_fix. */
int rvio_hip_get_fix_rows(rvio_hip* h, int instance, int32_t* m, int32_t* d, double* H, double* sigma);

/* --- past-frame fixes: a delayed fix fused at the frame it was taken (no reference counterpart) ----------------------------------- */
/* Every real source of absolute fixes is late: a relocalisation or fiducial result belongs to an image the filter consumed some frames ago, a
 * motion-capture pose crosses a network, a GNSS position arrives 50 - 200 ms after its epoch.  rvio_hip_update_fix fuses at the state it finds,
 * which is wrong by the platform's motion over the latency.  The robocentric window already holds what is needed: clone i (oldest first,
 * x[26 + 7 i ..]) = (q_i, p_i) is the relative pose between two consecutive image frames, C_i = R(q_i) rotating the older into the newer and p_i
 * the newer frame's origin in the older, and behind augment / compose the newest clone ends at the state's reference frame {R} — the IMU frame at
 * the newest image whose rvio_hip_augment_compose has run.  So the world pose of the IMU at any of the last n images is a function of (qG, pG) and
 * the newest clones (stochastic cloning), and fix_past_kernel (csrc/fix_past.hip, one wave per instance, the chain as an in-wave scan) linearises
 * the fix against it; aux_update_kernel, unchanged, runs right behind with m = 3 (POSE: 6) rows.
 * age a = 0 .. n: images back from {R}.  a = 0 is {R} itself, NOT the current IMU pose (qk, pk), which does not enter; behind a whole frame the
 * two coincide.  With R_G = R(x[0:4]), pG = x[4:7], l = lever:
 *   A_0 = I, t_0 = 0;   A_m = A_{m-1} C_{n-m},   t_m = t_{m-1} - A_m p_{n-m}   (m = 1 .. a);     u_a = t_a + A_a l,  s_a = u_a - pG
 *   POSITION  h_a = R_G^T s_a      r = z[0:3] - h_a
 *             cols 0-2: -R_G^T [s_a x]   3-5: -R_G^T   clone i = n - m (m = 1 .. a): 24+6i..: R_G^T [(u_a - t_{m-1}) x] A_{m-1}   27+6i..: -R_G^T A_m
 *   ATTITUDE  R(world -> IMU at that image) = A_a^T R_G;  E = R(z[3:7])^T A_a^T R_G,  r = (E21 - E12, E02 - E20, E10 - E01) / 2
 *             cols 0-2: R_G^T                          clone i = n - m (m = 1 .. a): 24+6i..: -R_G^T A_{m-1}
 *   POSE      the three position rows, then the three attitude rows
 * Every column not listed is exactly 0.0: columns 6 - 23 and every clone older than n - a.  RVIO_FIX_GRAVITY has no past form (it reads ba and
 * R_k g of now).
 * frac (POSITION only) = lam in [0, 1): the stamp lies lam of the way from the frame of age a towards the OLDER frame of age a + 1;
 * h = (1 - lam) h_a + lam h_{a+1} and H the same combination of the two row sets; lam > 0 needs a + 1 <= n.  ATTITUDE and POSE take frac = 0.
 * Host form: age and frac hold for every instance the call touches, and are checked here against the window, which is handle-wide.  _dev form:
 * d_age one int32 per instance (in a fleet every robot's latency differs), d_frac NULL (0) or one double per instance, d_fix / fix_stride /
 * d_active as in rvio_hip_update_fix_dev; nothing on the device is checked by the host.  An instance whose age is outside 0 .. n (or a + 1 > n
 * with lam > 0, lam outside [0, 1), lam > 0 with a kind other than POSITION) is written by neither launch and its record says so: m = 0,
 * applied = 0, img_count = -1, r = 0.  The kernel keeps an active flag of its own per instance (the caller's AND inside the window) and the
 * update runs on that.
 * rvio_hip_get_fix and rvio_hip_get_fix_rows report the last call of either family; rvio_fix_diag.img_count is here the count of the frame the
 * fix was fused against (the reference frame's count minus the age).  Everything rvio_hip_update_aux_dev documents holds: in place, `gate` as
 * there, the pose line rewritten, no ring record, a kept clone-block factor dropped, error bit 8 on a non-positive pivot.  The first call
 * allocates the fix block of rvio_hip_update_fix if need be, plus the flags and the staging of age / frac, outside the filter slab.
 * RVIO_ERR_STATE as rvio_hip_update_fix.  RVIO_ERR_INVALID: what rvio_hip_update_fix refuses, RVIO_FIX_GRAVITY, NULL d_age and — host form only —
 * frac outside [0, 1) or not 0 with a kind other than POSITION, an age outside 0 .. n, age + 1 > n with frac > 0 (rvio_hip_last_error).
 * NOT done: attitude interpolation, time-offset estimation, stamps newer than the last composed image (IMU bridging). */
int rvio_hip_update_fix_past(rvio_hip* h, int instance, int kind, int gate, int age, double frac, const rvio_fix* fix);
int rvio_hip_update_fix_past_dev(rvio_hip* h, int kind, int gate, const rvio_fix* d_fix, size_t fix_stride, const int32_t* d_age,
                                 const double* d_frac /* NULL: 0 */, const int32_t* d_active);
/* The age that the frame counted img_count (as rvio_odom.img_count and rvio_frame_info report it) has NOW: host arithmetic only, nothing is
 * waited for.  The handle counts a frame in rvio_hip_frame_plan and composes it in rvio_hip_augment_compose; between the two the newest count is
 * not composed yet.  RVIO_ERR_INVALID: NULL argument, no state, a frame not yet composed, a frame that has left the clone window. */
int rvio_hip_frame_age(rvio_hip* h, int img_count, int* age);

/* --- fixed-lag smoothed trajectory: pose and covariance of every frame of the clone window (no reference counterpart) ------------- */
/* rvio_hip_get_pose, the odometry ring and the IMU-rate rings publish the FILTER pose of the newest frame: frame k given measurements up to k.
 * The window holds better: clone i is the relative pose between two consecutive images, and every later camera update, delayed fix,
 * relative-pose measurement and map observation corrects it.  The world pose of the image `age` frames back, composed from (qG, pG) and the
 * newest `age` clones AS THEY ARE NOW, is a fixed-lag smoothed estimate, and its covariance follows from P — what a mapper, a loop-closure back
 * end, anything that stitches point clouds or key frames wants, `age` frames late.  window_pose_kernel (csrc/window_pose.hip, one workgroup per
 * (instance, age), FP64) forms it on the device; nothing of x or P crosses PCIe.
 * With the chain (A_m, t_m) of the past-fix table above, lever 0 and frac 0:
 *   p = R_G^T (t_a - pG)     the world position of the IMU at that image     R(q) = A_a^T R_G     world -> IMU at that image
 * in the frames and conventions of rvio_hip_get_pose; at age 0 they ARE that pose line (behind a whole frame).  The sign of q: at age 0 the
 * bits of x[0..3] (what rvio_odom.q carries); at age > 0 RotToQuat's (util/Numerics.h:126-167), normalised with q[3] >= 0.
 *   pose_cov = (C + C^T) / 2,  C = J P J^T,  J = the three POSITION rows (lever 0, frac 0) over the three ATTITUDE rows of the past-fix table at
 * age a: row-major 6 x 6 in the order and error convention of rvio_odom.pose_cov (x, y, z, then the world-frame rotation error phi), exactly
 * symmetric; at a = 0 J is rvio_odom's.
 * NOT done: cross-covariances between frames of the window IN THIS RECORD — rvio_hip_get_window_joint and rvio_hip_get_window_edges below
 * publish them, as the joint covariance of the poses and as between-factors; the pose of the frame that has just left the window;
 * time stamps in the record (the host knows the stamp of every img_count); interpolation between frames. */
typedef struct rvio_window_pose {   /* 368 bytes, no padding */
    int64_t seq;          /* smoothed-odometry ring: 1, 2, ... records written; rvio_hip_get_window*: 0 */
    int32_t img_count;    /* the count of the frame the record describes: the reference frame's count minus age (-1: age outside the window) */
    int32_t age;          /* images back from the state's reference frame */
    int32_t n_clones;     /* nCloneStates when the record was formed */
    int32_t reserved;     /* 0 */
    double p[3];
    double q[4];
    double pose_cov[36];
} rvio_window_pose;
/* The records of ages 0 .. min(n_clones, max_n - 1) of one instance, newest frame first, linearised at the state the call finds; *n = how many.
 * One launch on the filter stream; waits for the filter stream only, like rvio_hip_get_pose.  seq = 0.  The first call allocates its staging
 * (max_track_len records), outside the filter slab.  RVIO_ERR_STATE: no state yet (rvio_hip_set_state / rvio_hip_initialize);
 * RVIO_ERR_INVALID: NULL handle, out or n, instance out of range, max_n < 1 (rvio_hip_last_error). */
int rvio_hip_get_window(rvio_hip* h, int instance, int max_n, rvio_window_pose* out, int32_t* n);
/* Every instance, ages age_first .. age_first + n_ages - 1, into a device buffer: record (instance, age) lies at
 * d_out[instance * out_stride + age - age_first].  Asynchronous on the filter stream: nothing is waited for or read back.  An age beyond the
 * instance's window writes a record with img_count = -1, n_clones set and every other member 0.  RVIO_ERR_STATE: no state yet;
 * RVIO_ERR_INVALID: NULL handle or d_out, age_first < 0, n_ages outside 1 .. 65535, out_stride < n_ages.  (With a state handed in through
 * rvio_hip_set_state before any frame the reference frame's count is 0 and img_count = -age: tell such a record from one beyond the window by
 * its age, which is 0 there.) */
int rvio_hip_get_window_dev(rvio_hip* h, int age_first, int n_ages, rvio_window_pose* d_out, size_t out_stride);
/* The smoothed-odometry ring: behind the augmentation / composition stage of every path (and behind the odometry record, on the filter stream)
 * one record per instance of the frame `lag` images back, into a ring with exactly the capacity, layout, wrap, empty, stop and 1-GiB rules of
 * rvio_hip_set_odometry (capacity 0 .. 65536; 0 = off, the default: such a handle allocates and launches what it did before these entry points
 * existed).  lag = 0 .. max_track_len - 1; lag = max_track_len - 1 is the most-smoothed pose still in the window.  A frame is recorded only when
 * n_clones >= lag behind its stage: until the window has grown to `lag` there is no record and seq does not advance (the host knows the clone
 * count: nothing is read back to decide).  Another lag empties the ring like another capacity (seq restarts at 1); rvio_hip_initialize empties
 * it.  RVIO_ERR_INVALID: NULL handle, capacity outside 0 .. 65536, lag outside 0 .. max_track_len - 1 (rvio_hip_last_error);
 * RVIO_ERR_UNSUPPORTED: capacity x instances x 368 bytes exceeds 1 GiB. */
int rvio_hip_set_smoothed_odometry(rvio_hip* h, int capacity, int lag);
/* rvio_hip_get_odometry's and rvio_hip_get_odometry_all's clauses.  RVIO_ERR_STATE: the ring was never enabled. */
int rvio_hip_get_smoothed_odometry(rvio_hip* h, int instance, int64_t first_seq, int max_n, rvio_window_pose* out, int32_t* n);
int rvio_hip_get_smoothed_odometry_all(rvio_hip* h, rvio_window_pose* out /* batch records */, int64_t* seq);

/* --- pose-graph export: the edge between two frames of the window and the joint covariance of its poses (no reference counterpart) -- */
/* The records above carry the 6 x 6 MARGINAL covariance of each frame's world pose.  A pose-graph back end is not fed world poses with independent
 * marginals — the frames of one window are correlated almost perfectly through (qG, pG) — but BETWEEN-FACTORS: the relative pose of two frames
 * with the covariance of THAT quantity; and when it takes several frames at once it needs their JOINT covariance.  Both are formed on the device
 * (csrc/window_edge.hip); nothing of x or P crosses PCIe.  rvio_hip_update_rel puts a delta pose INTO the filter; this takes one OUT, in the same
 * conventions: an edge read here and handed back there (z = (p, q), sigma^2 = the diagonal of cov) means the same thing.
 * THE EDGE between the frames age_new = a and age_old = b images back, 0 <= a < b <= n_clones, with the chain (B_j, s_j) of the relative-pose table
 * below (k = b - a, lever 0); it depends on the clones n - b .. n - a - 1 and on nothing else of x, and on their square of P:
 *   p = -B_k^T s_k      the origin of frame a in frame b, along frame-b axes (the sense of a clone's p)
 *   R(q) = B_k          rotates frame b into frame a (the sense of a clone's q); RotToQuat's sign (util/Numerics.h:126-167), normalised, q[3] >= 0
 *   cov = (C + C^T) / 2,  C = H P H^T,  H = the six RVIO_REL_POSE rows of that table at lever 0: row-major 6 x 6, exactly symmetric.  Rows 0-2:
 * the error of p along frame-b axes (p_true = p + dp).  Rows 3-5: the rotation error along frame-a axes under R_true ~ (I - [dth x]) R(q) —
 * the order and convention in which rvio_hip_update_rel(RVIO_REL_POSE) takes sigma.  For b = a + 1 the edge IS clone n - b and cov is its
 * block of P with the two 3-blocks swapped (P holds rotation before position).  Formed directly from the clones of the span: the same covariance
 * taken from world-pose marginals and cross-covariances would subtract large, nearly equal numbers.
 * NOT done: the correlation between successive ring edges (they share no clone when their spans do not overlap, but P correlates every pair of
 * clones; rvio_hip_get_window_joint gives joint information instead); the frame that has already left the window; (qk, pk) as an endpoint;
 * information-matrix / g2o / GTSAM output (their quaternion order and perturbation side differ: convert on the host from the conventions above);
 * interpolation between frames. */
typedef struct rvio_window_edge {   /* 376 bytes, no padding */
    int64_t seq;            /* edge ring: 1, 2, ... records written; rvio_hip_get_window_edges*: 0 */
    int32_t img_count_new;  /* the reference frame's count minus age_new (-1: pair outside the window) */
    int32_t img_count_old;  /* the reference frame's count minus age_old */
    int32_t age_new, age_old;
    int32_t n_clones;       /* nCloneStates when the record was formed */
    int32_t reserved;       /* 0 */
    double p[3];
    double q[4];
    double cov[36];
} rvio_window_edge;
/* n_pairs edges of one instance, pair i = (age_new[i], age_old[i]) (host arrays) into out[i], linearised at the state the call finds.  One
 * launch on the filter stream; waits for the filter stream only.  seq = 0.  1 <= n_pairs <= 528 (every pair of the longest window); the first
 * call allocates its staging, outside the filter slab.  RVIO_ERR_STATE: no state yet; RVIO_ERR_INVALID: NULL handle or argument, instance out of
 * range, n_pairs outside 1 .. 528, a pair that is not 0 <= age_new < age_old <= n_clones (rvio_hip_last_error names it; nothing is launched). */
int rvio_hip_get_window_edges(rvio_hip* h, int instance, int n_pairs, const int32_t* age_new, const int32_t* age_old, rvio_window_edge* out);
/* Every instance, ONE pair list (device arrays) for all of them: record (instance, pair) lies at d_out[instance * out_stride + pair].
 * Asynchronous on the filter stream: nothing is waited for, read back or checked on the host.  A pair that is not 0 <= age_new < age_old <=
 * the instance's n_clones writes a record with img_count_new = -1, n_clones set and every other member 0.  RVIO_ERR_STATE: no state yet;
 * RVIO_ERR_INVALID: NULL handle or argument, n_pairs outside 1 .. 65535, out_stride < n_pairs. */
int rvio_hip_get_window_edges_dev(rvio_hip* h, int n_pairs, const int32_t* d_age_new, const int32_t* d_age_old, rvio_window_edge* d_out, size_t out_stride);
/* The edge-odometry ring: behind the smoothed record's place in every augmentation / composition stage, one record per instance of the pair
 * (age_new, age_old), into a ring with exactly the rules of rvio_hip_set_smoothed_odometry (capacity 0 .. 65536; 0 = off, the default: such a
 * handle allocates and launches what it did before these entry points existed).  A frame is recorded only when n_clones >= age_old behind its
 * stage.  (age_new, age_old) = (max_track_len - 2, max_track_len - 1) records the oldest clone behind every frame — each consecutive edge at
 * its most smoothed, just before it is marginalised: a back end's odometry chain.  Another pair empties the ring like another capacity (seq
 * restarts at 1); rvio_hip_initialize empties it.  RVIO_ERR_INVALID: NULL handle, capacity outside 0 .. 65536, a pair that is not
 * 0 <= age_new < age_old <= max_track_len - 1 (rvio_hip_last_error); RVIO_ERR_UNSUPPORTED: capacity x instances x 376 bytes exceeds 1 GiB. */
int rvio_hip_set_edge_odometry(rvio_hip* h, int capacity, int age_new, int age_old);
/* rvio_hip_get_odometry's and rvio_hip_get_odometry_all's clauses.  RVIO_ERR_STATE: the ring was never enabled. */
int rvio_hip_get_edge_odometry(rvio_hip* h, int instance, int64_t first_seq, int max_n, rvio_window_edge* out, int32_t* n);
int rvio_hip_get_edge_odometry_all(rvio_hip* h, rvio_window_edge* out /* batch records */, int64_t* seq);
/* THE JOINT COVARIANCE of the world poses of the ages 0 .. *n - 1, *n = min(n_clones + 1, max_n), frames newest first: with J_a the Jacobian of
 * rvio_window_pose at age a, block (a, b) of cov is J_a P J_b^T (6 x 6, pose_cov's order and error convention in rows and columns).  cov is
 * row-major with leading dimension ld >= 6 max_n; only rows and columns below 6 (*n) are written.  The diagonal blocks carry the bits of
 * rvio_window_pose.pose_cov, poses[a] the bits rvio_hip_get_window gives, and the whole matrix equals its transpose bit for bit.  max_n = m is
 * the leading 6 m x 6 m block of the full answer.  One launch on the filter stream; waits for that stream only; the first call allocates its
 * staging (at most 192^2 doubles and the records).  RVIO_ERR_STATE: no state yet; RVIO_ERR_INVALID: NULL handle, poses, cov or n, instance out
 * of range, max_n < 1, ld < 6 max_n. */
int rvio_hip_get_window_joint(rvio_hip* h, int instance, int max_n, rvio_window_pose* poses, double* cov, size_t ld, int32_t* n);
/* Every instance, ages 0 .. n_ages - 1: pose (instance, age) at d_poses[instance * pose_stride + age]; the instance's matrix, row-major with
 * leading dimension 6 n_ages, at d_cov + instance * cov_stride (doubles).  Asynchronous on the filter stream.  Blocks touching an age beyond an
 * instance's window are written as 0.0 and that age's pose record has the img_count = -1 form.  RVIO_ERR_STATE: no state yet; RVIO_ERR_INVALID:
 * NULL handle, d_poses or d_cov, n_ages outside 1 .. 32, pose_stride < n_ages, cov_stride < (6 n_ages)^2. */
int rvio_hip_get_window_joint_dev(rvio_hip* h, int n_ages, rvio_window_pose* d_poses, size_t pose_stride, double* d_cov, size_t cov_stride);

/* --- relative-pose measurements: a delta pose between two frames of the clone window (no reference counterpart) ------------------ */
/* What most other sensors on a robot produce is neither a state entry nor a world-frame fix but a DELTA POSE BETWEEN TWO INSTANTS: a wheel-odometry
 * integrator, lidar or radar scan matching, a second visual odometry, a loop closure inside the window, the statement "the platform did not move
 * between these two images".  Two world-frame fixes would inject absolute information the sensor never had, and rvio_hip_update_aux costs a
 * drain, a state read-back and a host Jacobian per measurement.  The robocentric window suits the measurement unusually well: clone i IS the
 * relative pose between two consecutive images, so the pose of the frame a images back in the frame b > a images back depends on the clones
 * n - b .. n - a - 1 only — not on (qG, pG), (qk, pk), velocity, biases or any newer or older clone.  rel_rows_kernel (csrc/rel_rows.hip, one
 * wave per instance, the chain as an in-wave scan like fix_past_kernel's) linearises the measurement there; aux_update_kernel, unchanged, runs
 * right behind with m = 3 (POSE: 6) rows.
 * Ages count images back from the reference frame {R} as in rvio_hip_update_fix_past: age_new = a, age_old = b, 0 <= a < b <= n, k = b - a.  With
 * C_i = R(q_i), l = lever (the sensed point in the IMU frame, the same at both instants) and i_j = n - a - j:
 *   B_0 = I, s_0 = 0;   B_j = B_{j-1} C_{i_j},   s_j = s_{j-1} - B_j p_{i_j}   (j = 1 .. k)
 * B_k rotates frame b into frame a (older into newer, the sense of a clone's q); -B_k^T s_k is the origin of frame a in frame b (newer in older,
 * the sense of a clone's p).  The record is rvio_fix as it stands:
 *   REL_POSITION  m = 3  h = B_k^T (l - s_k) - l: the displacement of the sensed point from instant b to instant a, in frame-b axes
 *                        r = z[0:3] - h;  sigma[0:3] lie along frame-b axes
 *                        clone i_j (j = 1 .. k): 24+6i..: -B_k^T [(l - s_{j-1}) x] B_{j-1}   27+6i..: B_k^T B_j
 *   REL_ATTITUDE  m = 3  z[3:7]: the quaternion rotating frame b into frame a;  E = B_k R(z[3:7])^T,  r = (E21 - E12, E02 - E20, E10 - E01) / 2
 *                        sigma[3:6] (rad) lie along frame-a axes
 *                        clone i_j (j = 1 .. k): 24+6i..: B_{j-1}                            27+6i..: 0
 *   REL_POSE      m = 6  the three position rows, then the three attitude rows
 * Every column not listed is exactly 0.0: all of columns 0 - 23 and every clone outside n - b .. n - a - 1.  For b = a + 1 without a lever the
 * measurement IS clone n - a - 1: h = p_i, z[3:7] ~ q_i, and the rows are two identity blocks.
 * Host form: the ages hold for every instance the call touches and are checked here against the window, which is handle-wide; the record is
 * checked as rvio_hip_update_fix checks it.  _dev form: d_age_new / d_age_old one int32 per instance, d_meas / meas_stride / d_active as in
 * rvio_hip_update_fix_dev; nothing on the device is checked by the host.  An instance whose ages are not 0 <= a < b <= n is written by neither
 * launch and its record says so: m = 0, applied = 0, img_count = -1, r = 0.  The kernel keeps an active flag of its own per instance (the
 * caller's AND inside the window) and the update runs on that.
 * rvio_hip_get_fix and rvio_hip_get_fix_rows report the last call of any of the three families; rvio_fix_diag.kind = 16 + the fix kind tells
 * this one apart, and rvio_fix_diag.img_count is the count of the NEWER frame (the reference frame's count minus age_new).  Everything
 * rvio_hip_update_aux_dev documents holds: in place, `gate` as there, the pose line rewritten, no ring record, a kept clone-block factor dropped,
 * error bit 8 on a non-positive pivot.  The first call allocates the fix block and the flags of rvio_hip_update_fix_past if need be, plus the
 * staging of the ages, outside the filter slab; a handle that never calls these allocates and launches what it did before.  Plain, batch and
 * sharded handles; on a sharded handle every rank calls alike.  rvio_hip_update_fix* and rvio_hip_update_fix_past* refuse these kinds.
 * RVIO_ERR_STATE as rvio_hip_update_fix.  RVIO_ERR_INVALID: NULL handle or record, a kind outside 16 .. 18, gate or instance out of range, NULL
 * d_age_new / d_age_old and — host form only — what rvio_hip_update_fix refuses of a record, age_new < 0, age_old > n, age_new >= age_old
 * (rvio_hip_last_error).
 * NOT done: interpolation between frames (both stamps are whole frames); the current (qk, pk) as an endpoint (age 0 is {R}); a sensor-to-IMU
 * rotation (the caller re-expresses a sensor's delta as the IMU's; only the lever arm is handled); correlation between successive overlapping
 * deltas of one integrator (they are treated as independent); time-offset estimation. */
typedef enum { RVIO_REL_POSITION = 16, RVIO_REL_ATTITUDE = 17, RVIO_REL_POSE = 18 } rvio_rel_kind;  /* = 16 + the fix kind: rvio_fix_diag.kind tells the families apart */
int rvio_hip_update_rel(rvio_hip* h, int instance, int kind, int gate, int age_new, int age_old, const rvio_fix* meas);
int rvio_hip_update_rel_dev(rvio_hip* h, int kind, int gate, const rvio_fix* d_meas, size_t meas_stride, const int32_t* d_age_new,
                            const int32_t* d_age_old, const int32_t* d_active);

/* --- map landmarks: pixel observations of KNOWN world points (no reference counterpart) ------------------------------------------ */
/* What a localisation user has is the observation of a known world point in an image: a surveyed marker corner, a fiducial's corners, a 2D-3D
 * match against a prior map.  Run through PnP on the host and handed over as RVIO_FIX_POSE, every point's information is squeezed through six
 * numbers with an invented covariance, and one wrong match poisons the whole pose.  The raw measurement is the pixel, and the handle owns what
 * linearises it: the instance's calibration, the tracker's undistortion and the chain of relative poses rvio_hip_update_fix_past walks, which
 * gives the camera pose AT THE IMAGE THE MATCH WAS MADE IN (matches always arrive late).  map_rows_kernel (csrc/map_rows.hip, one workgroup of
 * four waves per instance) forms two rows per point and a chi-square gate PER POINT against P as the call finds it; aux_update_kernel,
 * unchanged, runs right behind in RVIO_AUX_RESIDUAL mode with m = 2 n_max rows.
 * Frames and conventions are those of rvio_hip_update_fix_past: clone i holds (q_i, p_i), C_i = R(q_i); the age a = 0 .. n counts images back
 * from {R};  A_0 = I, t_0 = 0;  A_m = A_{m-1} C_{n-m},  t_m = t_{m-1} - A_m p_{n-m}.  With R_G = R(x[0:4]), pG = x[4:7], the world point
 * f = p_w and the instance's calibration (Rci, tci):
 *   w   = R_G f + pG                      the point in {R}
 *   p_I = A_a^T (w - t_a)                 in the IMU frame at the image `a` back
 *   p_C = Rci p_I + tci,  depth = p_C.z
 *   h   = (p_C.x / depth, p_C.y / depth)  normalised image coordinates
 *   r   = uv_n - h
 * With J = (1 / depth) [1 0 -h.x; 0 1 -h.y] and M = J Rci A_a^T (2 x 3) the two rows of a point are, under R_true ~ (I - [dth x]) R:
 *   cols 0-2 : M [(R_G f) x]          cols 3-5 : M
 *   clone i = n - m (m = 1 .. a):   24+6i.. (rotation): -M [(w - t_{m-1}) x] A_{m-1}     27+6i.. (position): M A_m
 * Every other column is exactly 0.0: columns 6 - 23 and every clone older than n - a.  (Held to central differences of h through the state
 * injection in tests/test_map_abi.py.)
 * units: RVIO_MAP_NORMALISED — uv holds undistorted normalised coordinates and both rows get sigma;  RVIO_MAP_PIXELS — uv holds raw pixels,
 * which the device casts to float and undistorts under the instance's calibration exactly as it does a tracked feature; the rows get
 * sigma / |fx| and sigma / |fy|.
 * Rows of a launch: slot j of an instance owns rows 2j and 2j + 1 of an m = 2 n_max stack (host form: n_max = n_obs).  A slot that is not used —
 * at or beyond the instance's count, rejected, gated out — has H = 0.0, r = 0.0, sigma = 1.0 in its rows: after whitening they are zero, S has a
 * unit diagonal there and they move nothing, so the update equals that of the compacted stack.
 * status of a slot (rvio_map_point): 0 used;  1 gated out;  2 rejected: depth < 0.1 m (csrc/launch_plan.h LP_MAP_MIN_DEPTH — a tuning value,
 * not a measurement), or a projection, residual or sigma that is not finite (a sigma not > 0 included);  3 empty slot.
 * gate_each = 1, the per-point gate: gamma_j = r~_j^T (H~_j P H~_j^T + I_2)^-1 r~_j on the whitened rows of slot j, kept iff
 * |gamma_j| < chi2inv(0.95, 2) — the table entry and the comparison of the feature gate; a non-positive pivot of the 2 x 2 refuses the slot
 * with status 1.  Every slot is gated independently against P as the call finds it.  With gate_each = 0, gamma_j is computed and reported all
 * the same.  gate = 1 is the stack gate of rvio_hip_update_aux against chi2inv(0.95, m): it counts the zeroed rows as degrees of freedom, so it
 * is LOOSER than nominal when slots are empty or refused, and one wrong match refuses the whole stack — prefer gate_each.
 * The kernel keeps an active flag per instance: the caller's flag AND the age inside 0 .. n AND at least one used slot; the update runs on that.
 * An instance with flag 0 is written by neither launch and its record says why: m = 0, applied = 0, and img_count = -1 for an age outside the
 * window (every slot then reads 3), n_used = 0 when every point was refused.  The host form's age holds for every instance the call touches,
 * like that of rvio_hip_update_fix_past.  _dev form: instance z reads d_obs + z * obs_stride records (0: shared), d_count[z] of them (NULL:
 * n_max each; clamped to 0 .. n_max) at the age d_age[z]; nothing on the device is checked by the host.
 * rvio_hip_get_map: the record and, if pts is not NULL, the RVIO_MAP_MAX_POINTS slot records of one instance from the last map call; gamma /
 * applied are those of the stack update.  rvio_hip_get_map_rows: m, d and (each may be NULL) the m x d rows, r and sigma as the device formed
 * them.  Both wait for the filter stream only.
 * Everything rvio_hip_update_aux_dev documents holds: in place, the pose line rewritten, no ring record, a kept clone-block factor dropped,
 * error bit 8 on a non-positive pivot of S.  The first call allocates the block of these calls outside the filter slab — rows at 16 x d_max per
 * instance, r, sigma, the records, the (gamma, applied) pairs, flags, staging; it is separate from the fix block: rvio_hip_get_fix* keep
 * reporting the last fix-family call.  A handle that never calls these allocates and launches what it did before.  Plain, batch and sharded
 * handles; on a sharded handle every rank calls alike.
 * RVIO_ERR_STATE as rvio_hip_update_fix.  RVIO_ERR_INVALID: a NULL handle or buffer (a NULL d_age included), n_obs / n_max outside 1 .. 8, units,
 * gate or gate_each outside their values, an instance out of range, an obs_stride below n_max unless it is 0, a window longer than the chain the
 * kernel holds and — host form only — a member that is not finite, sigma <= 0, an age outside 0 .. n (rvio_hip_last_error names the cause).
 * NOT done: estimating the camera-IMU extrinsic or a time offset; points whose world position is itself uncertain (a
 * per-point 3 x 3 prior); interpolation between frames; more than 8 points per launch (call again: sequential updates of independent
 * measurements are valid); alignment of a map frame to the filter's world frame — the frame of the pose line: anchored at the first IMU frame and, with
 * ini_enable_alignment, turned so that its z axis is the accelerometer's direction at rest — which is the caller's job, as for fixes.  Note on
 * gate_each: the gate is formed against P; a filter whose covariance does not admit its own drift refuses correct matches too (status 1,
 * n_used = 0), and a caller who trusts the matches — a relocalisation — calls with gate_each = 0. */
#define RVIO_MAP_MAX_POINTS 8                 /* 2 rows each = RVIO_AUX_MAX_ROWS */
typedef enum { RVIO_MAP_NORMALISED = 0, RVIO_MAP_PIXELS = 1 } rvio_map_units;
typedef struct rvio_map_obs { double p_w[3]; double uv[2]; double sigma; } rvio_map_obs;                                                  /* 48 B */
typedef struct rvio_map_point { double r[2]; double gamma; double depth; int32_t status, reserved; } rvio_map_point;                      /* 40 B */
typedef struct rvio_map_diag { double gamma; int32_t applied, m, n_used, n_obs, img_count, reserved; } rvio_map_diag;                     /* 32 B */
int rvio_hip_update_map(rvio_hip* h, int instance, int units, int gate, int gate_each, int age, int n_obs, const rvio_map_obs* obs);
int rvio_hip_update_map_dev(rvio_hip* h, int units, int gate, int gate_each, int n_max, const rvio_map_obs* d_obs, size_t obs_stride,
                            const int32_t* d_count, const int32_t* d_age, const int32_t* d_active);
int rvio_hip_get_map(rvio_hip* h, int instance, rvio_map_diag* out, rvio_map_point* pts);
int rvio_hip_get_map_rows(rvio_hip* h, int instance, int32_t* m, int32_t* d, double* H, double* r, double* sigma);

/* --- iterated measurement updates: relinearise the fix, past-fix, rel and map families (no reference counterpart) ----------------------- */
/* The four families above are non-linear in the robocentric state, and one linearisation is only good when the prior is close: a
 * relocalisation after drift is the far-from-prior case.  With max_iters = K > 1 a call of rvio_hip_update_fix / _fix_past / _rel / _map (and
 * their _dev forms) runs the iterated EKF update, a Gauss-Newton loop whose every pass refers to the PRIOR (x0, P0):
 *   dx_0 = 0, x_0 = x0
 *   pass i = 0 .. K - 1:   (H_i, r_i, sigma) = rows at x_i            the family's rows kernel, unchanged
 *                          v_i = r_i + H_i dx_i                        the residual referred to the prior
 *                          K_i = P0 H~_i^T (H~_i P0 H~_i^T + I)^-1     whitened rows, the arithmetic of rvio_hip_update_aux
 *                          dx_{i+1} = K_i v~_i,   step = max |dx_{i+1} - dx_i|
 *                          x_{i+1} = x0 (+) dx_{i+1}                   the state injection, always from x0, never chained
 *                          step < tol or i = K - 1:  P+ = the Joseph form with (K_i, H~_i) on P0; the instance is finished
 * K pairs (rows kernel, aux_iter_kernel — csrc/aux_update.hip, the update kernel with the four differences this needs) are enqueued on the filter
 * stream in a fixed sequence: no read-back, no host decision.  P is written once, on the final pass, so every pass forms its gain against P0;
 * x and the pose line are rewritten by every pass.  A per-instance running flag on the device — the caller's flag AND the rows kernel's own at
 * pass 0, cleared when the instance is finished — is what the kernels of the later passes get as their active flags: a finished instance keeps
 * the rows, records and state of the last pass that acted on it.
 * gate (the chi-square stack gate) is evaluated at pass 0 only, where v_0 is the innovation: a refused instance is finished with nothing
 * written.  A non-positive pivot at any pass sets sticky error bit 8 and leaves (x0, P0): x and the pose line are written back from the
 * snapshot, P is never touched, applied = 0.  Map calls: the per-point statuses and gammas are those pass 0 decided (a gated slot stays gated;
 * the per-point gate is formed at pass 0 only); a used slot whose depth falls below the limit at a later linearisation becomes rejected, and
 * if none is left the instance ends like a non-positive pivot.  gamma / applied of rvio_hip_get_fix / _get_map: pass 0's gamma; applied = 1
 * iff the last pass that ran wrote the state.
 * rvio_hip_set_meas_iterations: a handle setting like rvio_hip_set_standstill; max_iters 1 .. RVIO_MEAS_MAX_ITERS, tol >= 0 and finite
 * (0: always max_iters passes), else RVIO_ERR_INVALID with a message.  A handle that never calls it, or sets max_iters = 1, launches exactly
 * what it launched before: the plain kernels on the plain path, the same bits.  rvio_hip_update_aux[_dev] (caller-linearised rows) and
 * rvio_hip_standstill ignore the setting.  The first iterated call allocates the block outside the filter slab: per instance the snapshot
 * (26 + 7 n_max doubles and the pose line), dx (d_max doubles), the record and the running flag.
 * rvio_hip_get_meas_iter: passes run, the last step, converged (step < tol) and pass 0's gamma of one instance in the last fix / past-fix /
 * rel / map call; after a call at max_iters = 1: iterations = 1, step = 0, converged = 0, gamma0 = that call's gamma.  An instance the call
 * did not act on reads iterations = 0.  Waits for the filter stream only.  RVIO_ERR_STATE before the first such call.
 * NOT done: iterating the camera update; line search or damping; the Jacobian of the retraction at dx != 0. */
#define RVIO_MEAS_MAX_ITERS 8
typedef struct rvio_meas_iter { double step; double gamma0; int32_t iterations, converged; } rvio_meas_iter;                             /* 24 B */
int rvio_hip_set_meas_iterations(rvio_hip* h, int max_iters, double tol);
int rvio_hip_get_meas_iterations(rvio_hip* h, int* max_iters, double* tol);
int rvio_hip_get_meas_iter(rvio_hip* h, int instance, rvio_meas_iter* out);

/* --- feature-sharded updater (no reference counterpart) ------ */
/* Stage A: per-feature build + gate on the features f with f % world == rank,
 * then local compression to this shard's share of the information block
 * [A|b] = Hw^T [Hw | r], kept in two parts (the sum over the type-'2' features and the sum over
 * the type-'1' features) plus five counters, so that stage B can apply the reference's rank
 * truncation (Updater.cc:516-529) to the gathered whole.  *d_block is a device pointer owned by
 * the handle, *n_doubles its length: this is the payload of the all-gather, in the wire format of
 * csrc/rvio_dev.h shard_layout (r-vio_amd/abi.py shard_pack / shard_unpack mirror it): 8 counters, then
 * the 16 x 16 tiles (256 doubles each) on and above the diagonal of the type-'2' part that a
 * type-'2' feature can reach, then those of the type-'1' part — 8 + 256 (tiles2 + tiles1) doubles
 * for the CURRENT window (215 KB at 1600 features / 30 clones; rounds 2-5: 2 (6n_max+1)^2 doubles = 524 KB). */
int rvio_hip_update_local(rvio_hip* h, const rvio_tracks* tracks, int rank, int world,
                          double** d_block, int* n_doubles);
/* Stage B: sum `world` gathered blocks (device pointer, rank-major) in rank
 * order and run the EKF update; bit-identical on every rank. */
int rvio_hip_update_global(rvio_hip* h, const double* d_blocks, int world);

/* The whole sharded frame behind ONE call (what a multi-GPU host loop issues per image): rvio_hip_frame_begin_dev, rvio_hip_frame_plan,
 * rvio_hip_update_local, ncclAllGather of the blocks ON THE HANDLE'S FILTER STREAM, rvio_hip_update_global, rvio_hip_augment_compose,
 * rvio_hip_frame_end — no host synchronisation, the collective ordered by plain stream order.  `comm` is the caller's ncclComm_t (RCCL);
 * NULL is allowed with world == 1 only (no collective).  `allgather` = NULL: RCCL's ncclAllGather is resolved from the RCCL the process has
 * loaded (the library has no link-time dependency on it); or the entry point itself,
 *   int (*)(const void* send, void* recv, size_t count, int dtype, void* comm, hipStream_t stream). */
int rvio_hip_frame_sharded_dev(rvio_hip* h, const uint8_t* d_img, int stride, const rvio_imu* d_imu, int m,
                               const float* d_cand_xy, int n_cand, int rank, int world, void* comm, void* allgather);

/* --- diagnostics for parity tests ------------------------------------------ */
/* per-feature results of the last update: accept flag, Mahalanobis distance,
 * nDOF, inverse-depth estimate (phi,psi,rho). arrays sized n_feat. */
int rvio_hip_get_update_diag(rvio_hip* h, int32_t* n_feat, int32_t* accepted, double* gamma,
                             int32_t* ndof, double* pfinv /* n_feat x 3 */);

/* --- landmark cloud ---------------------------------------------------------- */
/* Updater::update's landmark cloud (Updater.cc:78-87,430-448,458). Off by default; takes effect from the next update enqueued;
 * on a batch handle for every instance.  The first enable drains the handle and allocates the cloud's buffers; with the cloud off a
 * handle launches what it launched before.  One cloud per update call, also when the update itself is then skipped (<= 2 accepted
 * features) and when it is empty; frames without an update leave the last cloud in place. */
int rvio_hip_set_landmarks(rvio_hip* h, int enable);
/* The cloud of the most recent update: n points, frame = nImageCountAfterInit when that update was issued (-1: none since create /
 * rvio_hip_initialize), feat[i] = index in that frame's hand-over list (ascending), p_r = points in {Rk} as published, p_world =
 * R(qG)^T (p_r - pG) with the updated state. Buffers hold ceil(n_features/2) entries; any pointer may be NULL. Synchronises like
 * the other getters. RVIO_ERR_STATE if the cloud was never enabled. Batch handle: instance 0 (_at: any instance; RVIO_ERR_INVALID
 * out of range).  rvio_hip_initialize clears the cloud (n = 0, frame = -1) and keeps the enable flag.
 * A point is a feature that passed the chi^2 gate (Updater.cc:422) with rho > 0 (Updater.cc:430): rank-truncated type-'1' features
 * are in it, a feature accepted with rho = 0 is not.  p_r = R_k (R_ic e / rho + t_ic) + t_k, (R_k, t_k) the end of the feature's
 * relative-pose chain in xk1k (Updater.cc:114-131).
 * Feature-sharded handles (rvio_hip_update_local / _global, rvio_hip_frame_sharded_dev): the cloud is what THIS rank's per-feature
 * stage accepted — the features f with f % world == rank, except for an update handed at most 24 features (the literal path,
 * csrc/literal.h LIT_FEATS), where every rank builds every feature and so holds the whole cloud.  `feat` lets a caller merge the
 * ranks' clouds; p_world is the same on every rank (the updated state is replicated).  The all-gather payload carries no cloud. */
int rvio_hip_get_landmarks(rvio_hip* h, int32_t* n, int32_t* frame, int32_t* feat, double* p_r, double* p_world);
int rvio_hip_get_landmarks_at(rvio_hip* h, int instance, int32_t* n, int32_t* frame, int32_t* feat, double* p_r, double* p_world);

/* --- landmark covariance ------------------------------------------------------ */
/* The 3 x 3 uncertainty of every point of the cloud, formed on the device behind the cloud (csrc/landmark_cov.hip).  The reference
 * publishes none.  One record per cloud point, in the cloud's order; 224 bytes, no padding.
 *
 * The quantity.  theta = (phi, psi, rho), the inverse-depth estimate in the track's first camera frame, is not a state: it is the
 * least-squares solution of ALL L observations of the track given the clones (for a type-'2' track too: the halving of
 * Updater.cc:271-275 concerns the update, not the triangulation).  With Hf (2L x 3) and Hx (2L x 6 nPh, nPh = L - 1) the raw
 * measurement Jacobians before the nullspace projection, evaluated at the stored estimate, N = Hf^T Hf, A = N^-1 Hf^T and pixel noise
 * n ~ sigma^2 I (sigma = max(sigma_px, sigma_py), the normalised sigma the update itself uses), to first order
 *     dtheta = -A (Hx dx + n).
 * The published point is p_r = g(theta, x-) = R_k (R_ic e(theta) / rho + t_ic) + t_k.  With Jth = dg/dtheta, Jx = dg/d(clone errors)
 * and M = Jx - Jth A Hx:
 *     cov_r = sigma^2 Jth N^-1 Jth^T + M P-_span M^T
 * where (x-, P-) are the state and covariance the update READ (the prior pair), P-_span the rows / columns of the track's clones.
 * This is exact to first order for that pair, because n is independent of the prior error.
 *
 * Frames.  p_r, cov_r: the frame {R} of the cloud (the IMU frame at the end of the track's relative-pose chain), the bits of
 * rvio_hip_get_landmarks' p_r.  p_w, cov_w: p_w = R(qG-)^T (p_r - pG-) evaluated WHOLLY at the prior state x- — NOT the cloud's
 * p_world, which uses the updated (qG, pG) — and cov_w the same formula with M_w = R_G^T [dp_w/dthG, dp_w/dpG | M] over the columns
 * 0 .. 5 of P- and the span, cross blocks included.  Error convention: that of P (R_true ~ (I - [dth x]) R on every rotation,
 * positions additive); both covariances are row-major and symmetric bit for bit.
 *
 * rho_sigma = sqrt(Cov(theta)_22) of the same formula, Cov(theta) = sigma^2 N^-1 + (A Hx) P-_span (A Hx)^T: the cheap parallax test.
 * status: 0 ok; 1: N is not positive definite to working precision (a Cholesky pivot at or below 64 * 2^-52 of its diagonal entry,
 * also a non-positive one) — cov_r, cov_w and rho_sigma are NaN, p_r and p_w are still filled.
 *
 * NOT done: the posterior-refined landmark theta - A Hx dx and its covariance with P+; a covariance for the cloud's own mixed
 * p_world (prior clones, posterior (qG, pG)): it needs Cov(dx+, dx-) = (I - K H) P-, which no buffer holds; cross-covariance between
 * a landmark and the window poses, or between landmarks; a ring of clouds; time stamps in the record; uncertain map points in
 * rvio_hip_update_map. */
typedef struct rvio_landmark_cov {
    int32_t feat;        /* index in the frame's hand-over list: rvio_hip_get_landmarks' feat */
    int32_t n_obs;       /* L: the observations of the track */
    int32_t status;      /* 0 ok, 1 N not positive definite */
    int32_t reserved;    /* 0 */
    double rho;          /* the inverse depth in the first camera frame */
    double rho_sigma;
    double p_r[3];
    double p_w[3];
    double cov_r[9];
    double cov_w[9];
} rvio_landmark_cov;
/* Off by default.  Enabling it enables the cloud if that is off; switching the cloud off switches this off.  The first enable drains
 * the handle and allocates ceil(n_features/2) records per instance; takes effect from the next update enqueued, on a batch handle for
 * every instance.  The kernel only reads the filter's buffers: (x, P), the cloud and every ring are bit-identical with and without
 * it, and a handle that does not enable it launches what it launched before. */
int rvio_hip_set_landmark_cov(rvio_hip* h, int enable);
/* The records of the most recent cloud: rvio_hip_get_landmarks' rules — n and frame are the cloud's, rec holds ceil(n_features/2)
 * entries (may be NULL), rvio_hip_initialize clears (n = 0, frame = -1), RVIO_ERR_STATE if the covariance was never enabled,
 * RVIO_ERR_INVALID for an instance out of range.  A cloud published while the covariance was switched off has no records: n = 0
 * under the stamp of the last cloud that has.  Feature-sharded handles: each rank covers its own cloud, as documented there. */
int rvio_hip_get_landmark_cov(rvio_hip* h, int32_t* n, int32_t* frame, rvio_landmark_cov* rec);
int rvio_hip_get_landmark_cov_at(rvio_hip* h, int instance, int32_t* n, int32_t* frame, rvio_landmark_cov* rec);
/* Every instance into the caller's DEVICE buffers, enqueued on the handle's stream, nothing waited for: instance i's records from
 * d_out[i * out_stride] on (out_stride >= ceil(n_features/2) records), its count into d_count[i] (may be NULL).  Records at and
 * beyond the count are not meaningful. */
int rvio_hip_get_landmark_cov_dev(rvio_hip* h, rvio_landmark_cov* d_out, size_t out_stride, int32_t* d_count);

/* pyramid level of the most recent image (u8 w*h, int16 (dx,dy) w*h*2) and the raw KLT output
 * (vFeatsTracked + its undistorted-normalised form) of the last track() call */
int rvio_hip_debug_pyramid(rvio_hip* h, int level, int32_t* w, int32_t* hgt, uint8_t* img, int16_t* dxy);
int rvio_hip_debug_tracked(rvio_hip* h, int n, float* xy, float* un_xy);
/* Measurement hook for bench.py's roofline object: average device time (us, HIP events on the handle's stream)
 * of `iters` back-to-back launches of one hot kernel on the operands the last frame left in HBM.
 * which: 0 = solve kernel, 1 = KLT kernel (the current image matched back onto the previous one from the current feature positions),
 * 2 = per-feature Jacobian/nullspace/gate kernel, 3 = reduction of the per-feature information shares (+ rank truncation),
 * 4 = U/G/P1 strips, 5 = Joseph-form kernel (4, 5: the two-launch forms), 6 = cornerSubPix on the last corner list,
 * 7 = U/G/P1 + Joseph form as this handle launches them for an update (one instance, 6n <= 60: one fused kernel),
 * 8 = the per-feature kernel with propagate fused in, as the pipelined frame launches it, 9 = the detector's selection kernel,
 * 10 = the landmark cloud kernel on the hand-over table and per-feature results of the last update (into buffers of its own: the
 * cloud rvio_hip_get_landmarks returns is left alone; RVIO_ERR_UNSUPPORTED unless the cloud was enabled),
 * 11 = the gray conversion of the last image handed over, in the form the frame launched (a _dev entry point: the caller's image must
 * still be alive; RVIO_ERR_UNSUPPORTED without a colour format or before the first image),
 * 12 = the odometry record kernel on the composed state the last frame left, all instances (into a slot of its own: the ring is left alone;
 * RVIO_ERR_UNSUPPORTED unless the ring was enabled),
 * 13 = the IMU-pose kernel on the state and the IMU batch of the last frame, all instances (a _dev entry point: the caller's IMU buffer must
 * still be alive; into a buffer of its own; RVIO_ERR_UNSUPPORTED unless the IMU-rate ring was enabled and a frame has propagated),
 * 14 = the IMU-covariance kernel as the ring launches it, on the same operands, into a buffer of its own (RVIO_ERR_UNSUPPORTED under 13's
 * conditions, or when the covariance ring is off),
 * 15 = the landmark-covariance kernel as the update launches it, on the cloud and operands of the last update, all instances (into records
 * of its own; RVIO_ERR_UNSUPPORTED unless rvio_hip_set_landmark_cov was enabled and a cloud has been published). */
int rvio_hip_debug_time_kernel(rvio_hip* h, int which, int iters, float* avg_us);
/* Test hook against results that depend on LEFT-OVER state (scratch in HBM, LDS contents, stale hand-over entries).  Drains every stream of
 * the handle, then: what & 1 fills the filter's scratch and the spare state / covariance buffer with 0xff bytes (NaN); & 2 rewrites the LDS
 * of the whole chip with NaN patterns; & 4 does the same to the Tracker -> Updater hand-over tables (types / len / meas; counts stay), the
 * tracker's per-frame scratch and the gray buffers of a colour handle; & 8 sets the device-side error bit 4 ("a stage counter timed out", RVIO_ERR_STATE at the next
 * rvio_hip_sync) so that the recovery path — rvio_hip_initialize — can be exercised.  1 | 2 | 4 between the frames of a sequence must not
 * change any result. */
int rvio_hip_debug_poison(rvio_hip* h, int what);
/* Test hook against ordering holes between the handle's streams: occupies stream `which` (0 filter, 1 tracker / image chain 0, 2 side stream
 * — KLT, RANSAC, book-keeping —, 3 image chain 1) with a sleeping one-wave kernel for `usec` microseconds, enqueued where the call is made.
 * A frame sequence with stalls sprinkled over the streams must give the results of the synchronised run bit for bit. */
int rvio_hip_debug_stall(rvio_hip* h, int which, int usec);
/* Test hook against timing dependence inside kernels: `wgs` workgroups on a stream of their own load HBM, L2 and LDS for `usec`
 * microseconds beside whatever the handle has in flight (a box under load); results must not move by a bit. */
int rvio_hip_debug_noise(rvio_hip* h, int wgs, int usec);
/* Test hook: selects the throughput forms of the image kernels (the ones a batch handle of >= 8 instances launches: several pixels per
 * thread, four corners / features per wave) on any handle, or the latency forms (0) on a batch handle.  The two families compute the same
 * bits by construction; the tests run the KLT early-out cases and the detector's image set through both. */
int rvio_hip_debug_kernel_forms(rvio_hip* h, int throughput);

#ifdef __cplusplus
}
#endif
#endif /* RVIO_HIP_H */
