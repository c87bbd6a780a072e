"""Loader + thin ctypes wrapper of librvio_hip.so (the C-ABI of include/rvio_hip.h).

There is NO CPU fallback: if the HIP library is missing, cannot be loaded, or no
GPU is present, every entry point raises.
"""
import ctypes as C
import os
import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RVIO_HIP_LIB", os.path.join(HERE, "librvio_hip.so"))   # override: A/B kernel experiments

# every symbol include/rvio_hip.h declares (tests/test_abi.py checks the export list)
SYMBOLS = [
    "rvio_config_euroc", "rvio_hip_create", "rvio_hip_destroy", "rvio_hip_last_error", "rvio_hip_abi_version",
    "rvio_hip_stream", "rvio_hip_sync", "rvio_hip_set_state", "rvio_hip_get_state", "rvio_hip_initialize",
    "rvio_hip_propagate", "rvio_hip_update", "rvio_hip_augment_compose", "rvio_hip_track", "rvio_hip_track_dev",
    "rvio_hip_track_points", "rvio_hip_get_tracks", "rvio_hip_get_tracker_points", "rvio_hip_update_tracked",
    "rvio_hip_frame", "rvio_hip_frame_dev", "rvio_hip_frame_points", "rvio_hip_get_frame_info", "rvio_hip_get_pose",
    "rvio_hip_update_local", "rvio_hip_update_global", "rvio_hip_get_update_diag",
    "rvio_hip_debug_pyramid", "rvio_hip_debug_tracked", "rvio_hip_frame_plan", "rvio_hip_propagate_dev",
    "rvio_hip_debug_time_kernel", "rvio_hip_get_corners", "rvio_hip_frame_begin_dev", "rvio_hip_frame_end",
    "rvio_hip_create_batch", "rvio_hip_batch_size", "rvio_hip_set_state_at", "rvio_hip_get_state_at", "rvio_hip_frame_tracks_dev",
    "rvio_hip_frame_batch_dev", "rvio_hip_get_tracker_points_at", "rvio_hip_frame_sharded_dev", "rvio_hip_debug_poison", "rvio_hip_debug_stall", "rvio_hip_debug_noise", "rvio_hip_debug_kernel_forms",
    "rvio_hip_set_landmarks", "rvio_hip_get_landmarks", "rvio_hip_get_landmarks_at",
    "rvio_hip_set_landmark_cov", "rvio_hip_get_landmark_cov", "rvio_hip_get_landmark_cov_at", "rvio_hip_get_landmark_cov_dev",
    "rvio_hip_set_image_format", "rvio_hip_get_image_format",
    "rvio_hip_set_odometry", "rvio_hip_get_odometry", "rvio_hip_get_odometry_all", "rvio_hip_get_pose_at",
    "rvio_calibration_from_config", "rvio_hip_set_calibration_at", "rvio_hip_set_calibrations", "rvio_hip_get_calibration_at", "rvio_hip_initialize_at",
    "rvio_hip_predict", "rvio_hip_predict_dev", "rvio_hip_set_imu_odometry", "rvio_hip_get_imu_odometry",
    "rvio_hip_update_aux", "rvio_hip_update_aux_dev", "rvio_hip_get_aux_diag",
    "rvio_hip_predict_cov", "rvio_hip_predict_cov_dev", "rvio_hip_set_imu_odometry_cov", "rvio_hip_get_imu_odometry_cov",
    "rvio_standstill_config_default", "rvio_hip_set_standstill", "rvio_hip_standstill", "rvio_hip_standstill_dev", "rvio_hip_get_standstill",
    "rvio_hip_update_fix", "rvio_hip_update_fix_dev", "rvio_hip_get_fix", "rvio_hip_get_fix_rows",
    "rvio_hip_update_fix_past", "rvio_hip_update_fix_past_dev", "rvio_hip_frame_age",
    "rvio_hip_get_window", "rvio_hip_get_window_dev", "rvio_hip_set_smoothed_odometry", "rvio_hip_get_smoothed_odometry", "rvio_hip_get_smoothed_odometry_all",
    "rvio_hip_get_window_edges", "rvio_hip_get_window_edges_dev", "rvio_hip_set_edge_odometry", "rvio_hip_get_edge_odometry", "rvio_hip_get_edge_odometry_all",
    "rvio_hip_get_window_joint", "rvio_hip_get_window_joint_dev",
    "rvio_hip_update_rel", "rvio_hip_update_rel_dev",
    "rvio_hip_update_map", "rvio_hip_update_map_dev", "rvio_hip_get_map", "rvio_hip_get_map_rows",
    "rvio_hip_set_meas_iterations", "rvio_hip_get_meas_iterations", "rvio_hip_get_meas_iter",
]

_LIB = None
dp, fp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_ubyte)


class RvioHipError(RuntimeError):
    pass


def load():
    """dlopen the in-tree HIP library; fail loudly when it is absent."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RvioHipError("librvio_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(no CPU fallback exists for the product path)")
        try:
            import torch  # noqa: F401  when torch is used in the same process its bundled HIP runtime has to be loaded first
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        # the version first: a library built from an older header must fail HERE, with a sentence, not at the first missing symbol
        L.rvio_hip_abi_version.restype = C.c_int
        if L.rvio_hip_abi_version() != abi.ABI_VERSION:
            raise RvioHipError("%s speaks ABI %d, this binding expects %d (include/rvio_hip.h): rebuild it — python -c 'import __graft_entry__ as g; g.build()'"
                               % (LIB_PATH, L.rvio_hip_abi_version(), abi.ABI_VERSION))
        L.rvio_hip_last_error.restype = C.c_char_p
        L.rvio_hip_last_error.argtypes = [C.c_void_p]
        L.rvio_hip_stream.restype = C.c_void_p
        L.rvio_hip_stream.argtypes = [C.c_void_p]
        L.rvio_hip_destroy.argtypes = [C.c_void_p]
        L.rvio_hip_destroy.restype = None
        _LIB = L
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


class RvioHip:
    """One filter instance on one GPU (mirrors the System-owned stage objects, System.h:89-92)."""

    def __init__(self, cfg, device=0, batch=None, front_end=False):
        """batch=B: B independent instances behind one handle (rvio_hip_create_batch); front_end: with the tracker, else filter only"""
        self.L = load()
        self.cfg = cfg
        self.h = C.c_void_p()
        self.batch = 1 if batch is None else int(batch)
        if batch is None:
            rc = self.L.rvio_hip_create(C.byref(cfg), int(device), C.byref(self.h))
        else:
            rc = self.L.rvio_hip_create_batch(C.byref(cfg), int(device), int(batch), int(bool(front_end)), C.byref(self.h))
        if rc != 0:
            msg = self.L.rvio_hip_last_error(self.h).decode() if self.h else ""
            if self.h:
                self.L.rvio_hip_destroy(self.h)
                self.h = C.c_void_p()
            raise RvioHipError("rvio_hip_create failed: rc=%d %s" % (rc, msg))
        self.nmax = cfg.max_track_len - 1
        self.Fu = abi.fu(cfg)
        self.channels = 1
        self.sample_dtype = "uint8"

    def close(self):
        if getattr(self, "h", None):
            self.L.rvio_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise RvioHipError("%s failed: rc=%d %s" % (what, rc, self.L.rvio_hip_last_error(self.h).decode()))

    def sync(self):
        self._ck(self.L.rvio_hip_sync(self.h), "sync")

    def stream(self):
        return self.L.rvio_hip_stream(self.h)

    # ---- state
    def set_state(self, x, P):
        x = np.ascontiguousarray(x, float)
        Pf = np.asfortranarray(P, dtype=float)
        self._ck(self.L.rvio_hip_set_state(self.h, _p(x, dp), len(x), Pf.ctypes.data_as(dp), P.shape[0]), "set_state")

    def get_state(self):
        xb = np.zeros(26 + 7 * (self.nmax + 1))
        Pb = np.zeros((24 + 6 * (self.nmax + 1)) ** 2)
        xd, d = C.c_int(0), C.c_int(0)
        self._ck(self.L.rvio_hip_get_state(self.h, _p(xb, dp), C.byref(xd), _p(Pb, dp), C.byref(d)), "get_state")
        return xb[: xd.value].copy(), Pb[: d.value ** 2].reshape(d.value, d.value, order="F").copy()

    def set_state_at(self, i, x, P):
        x = np.ascontiguousarray(x, float)
        Pf = np.asfortranarray(P, dtype=float)
        self._ck(self.L.rvio_hip_set_state_at(self.h, int(i), _p(x, dp), len(x), Pf.ctypes.data_as(dp), P.shape[0]), "set_state_at")

    def get_state_at(self, i):
        xb = np.zeros(26 + 7 * (self.nmax + 1))
        Pb = np.zeros((24 + 6 * (self.nmax + 1)) ** 2)
        xd, d = C.c_int(0), C.c_int(0)
        self._ck(self.L.rvio_hip_get_state_at(self.h, int(i), _p(xb, dp), C.byref(xd), _p(Pb, dp), C.byref(d)), "get_state_at")
        return xb[: xd.value].copy(), Pb[: d.value ** 2].reshape(d.value, d.value, order="F").copy()

    def frame_tracks_dev(self, d_imu_ptr, imu_stride, m, d_n_feat_ptr, d_types_ptr, d_len_ptr, d_meas_ptr):
        """MonoVIO body after the tracker on device-resident hand-over tables, all instances in one launch per stage"""
        self._ck(self.L.rvio_hip_frame_tracks_dev(self.h, C.c_void_p(d_imu_ptr), int(imu_stride), int(m), C.c_void_p(d_n_feat_ptr),
                                                  C.c_void_p(d_types_ptr), C.c_void_p(d_len_ptr), C.c_void_p(d_meas_ptr)), "frame_tracks_dev")

    def frame_batch_dev(self, d_imgs_ptr, stride, img_stride, d_imu_ptr, imu_stride, m):
        """one camera frame of every instance of a batch handle with front end (device detector)"""
        self._ck(self.L.rvio_hip_frame_batch_dev(self.h, C.c_void_p(d_imgs_ptr), int(stride), C.c_size_t(int(img_stride)), C.c_void_p(d_imu_ptr),
                                                 int(imu_stride), int(m)), "frame_batch_dev")

    def initialize(self, w, a, n_imu):
        w = np.ascontiguousarray(w, float)
        a = np.ascontiguousarray(a, float)
        self._ck(self.L.rvio_hip_initialize(self.h, _p(w, dp), _p(a, dp), int(n_imu)), "initialize")

    def initialize_at(self, i, w, a, n_imu):
        """System::initialize for instance i alone (its own gravity direction and biases); before the first frame, no handle-wide reset"""
        w = np.ascontiguousarray(w, float)
        a = np.ascontiguousarray(a, float)
        self._ck(self.L.rvio_hip_initialize_at(self.h, int(i), _p(w, dp), _p(a, dp), int(n_imu)), "initialize_at")

    # ---- per-instance calibration (intrinsics, distortion model, camera-IMU extrinsic)
    def set_calibration_at(self, i, cal):
        """instance i computes with abi.rvio_calibration `cal` from the next call on (drains the handle; call it before the first frame)"""
        self._ck(self.L.rvio_hip_set_calibration_at(self.h, int(i), C.byref(cal)), "set_calibration_at")

    def set_calibrations(self, cals):
        """one abi.rvio_calibration per instance, uploaded in one copy"""
        cals = list(cals)
        if len(cals) != self.batch:
            raise RvioHipError("set_calibrations: %d calibrations for %d instances" % (len(cals), self.batch))
        arr = (abi.rvio_calibration * self.batch)(*cals)
        self._ck(self.L.rvio_hip_set_calibrations(self.h, arr), "set_calibrations")

    def get_calibration_at(self, i):
        cal = abi.rvio_calibration()
        self._ck(self.L.rvio_hip_get_calibration_at(self.h, int(i), C.byref(cal)), "get_calibration_at")
        return cal

    # ---- stages
    def propagate(self, imu):
        imu = np.ascontiguousarray(imu)
        self._ck(self.L.rvio_hip_propagate(self.h, imu.ctypes.data_as(C.POINTER(abi.rvio_imu)), len(imu)), "propagate")

    def update(self, types, lens, meas):
        tr = abi.make_tracks(types, lens, meas)
        self._ck(self.L.rvio_hip_update(self.h, C.byref(tr)), "update")

    def update_tracked(self):
        self._ck(self.L.rvio_hip_update_tracked(self.h), "update_tracked")

    def update_local(self, types, lens, meas, rank, world):
        """returns (device pointer, n_doubles) of this rank's [A|b] block"""
        tr = abi.make_tracks(types, lens, meas)
        ptr, n = dp(), C.c_int(0)
        self._ck(self.L.rvio_hip_update_local(self.h, C.byref(tr), rank, world, C.byref(ptr), C.byref(n)), "update_local")
        return C.cast(ptr, C.c_void_p).value, n.value

    def update_global(self, d_blocks_ptr, world):
        self._ck(self.L.rvio_hip_update_global(self.h, C.c_void_p(d_blocks_ptr), world), "update_global")

    def update_diag(self):
        nf = C.c_int32(0)
        acc, gam, ndof, pf = np.zeros(self.Fu, np.int32), np.zeros(self.Fu), np.zeros(self.Fu, np.int32), np.zeros((self.Fu, 3))
        self._ck(self.L.rvio_hip_get_update_diag(self.h, C.byref(nf), _p(acc, ip), _p(gam, dp), _p(ndof, ip), _p(pf, dp)), "update_diag")
        n = nf.value
        return dict(accepted=acc[:n], gamma=gam[:n], ndof=ndof[:n], pfinv=pf[:n])

    # ---- landmark cloud (Updater.cc:78-87,430-448,458)
    def set_landmarks(self, on=True):
        """compute Updater::update's landmark cloud behind every update from the next one on (all instances of a batch handle)"""
        self._ck(self.L.rvio_hip_set_landmarks(self.h, int(bool(on))), "set_landmarks")

    def landmarks_at(self, i):
        """the cloud of the most recent update of instance i: dict(n, frame, feat, p_r, p_world), arrays cut to n"""
        n, frame = C.c_int32(0), C.c_int32(0)
        feat, pr, pw = np.zeros(self.Fu, np.int32), np.zeros((self.Fu, 3)), np.zeros((self.Fu, 3))
        self._ck(self.L.rvio_hip_get_landmarks_at(self.h, int(i), C.byref(n), C.byref(frame), _p(feat, ip), _p(pr, dp), _p(pw, dp)),
                 "get_landmarks_at")
        k = n.value
        return dict(n=k, frame=frame.value, feat=feat[:k].copy(), p_r=pr[:k].copy(), p_world=pw[:k].copy())

    def landmarks(self):
        return self.landmarks_at(0)

    # ---- landmark covariance (csrc/landmark_cov.hip): the 3 x 3 uncertainty of every cloud point
    def set_landmark_cov(self, on=True):
        """form an rvio_landmark_cov record per cloud point behind every update from the next one on (switches the cloud on if it is off)"""
        self._ck(self.L.rvio_hip_set_landmark_cov(self.h, int(bool(on))), "set_landmark_cov")

    def landmark_cov_at(self, i):
        """the records of the most recent cloud of instance i: dict(n, frame, rec), rec an array of abi.LANDMARK_COV_DTYPE cut to n"""
        n, frame = C.c_int32(0), C.c_int32(0)
        rec = np.zeros(self.Fu, abi.LANDMARK_COV_DTYPE)
        self._ck(self.L.rvio_hip_get_landmark_cov_at(self.h, int(i), C.byref(n), C.byref(frame), C.c_void_p(rec.ctypes.data)), "get_landmark_cov_at")
        return dict(n=n.value, frame=frame.value, rec=rec[:n.value].copy())

    def landmark_cov(self):
        return self.landmark_cov_at(0)

    def landmark_cov_dev(self, d_out_ptr, out_stride, d_count_ptr=None):
        """every instance's records (and counts) into the caller's device buffers, enqueued on the handle's stream, nothing waited for"""
        self._ck(self.L.rvio_hip_get_landmark_cov_dev(self.h, C.c_void_p(d_out_ptr), C.c_size_t(out_stride), C.c_void_p(d_count_ptr or 0)),
                 "get_landmark_cov_dev")

    def augment_compose(self, do_augment=True):
        self._ck(self.L.rvio_hip_augment_compose(self.h, int(do_augment)), "augment_compose")

    # ---- front end
    @staticmethod
    def _cand(cand):
        """(pointer, count) of a corner list; None selects the device detector"""
        if cand is None:
            return None, 0, None
        cand = np.ascontiguousarray(cand, np.float32)
        return _p(cand, fp), len(cand), cand

    # ---- colour cameras (Tracker.cc:182-196)
    def set_image_format(self, fmt):
        """abi.RVIO_PIX_*: what img / d_img of the image entry points hold from the next image on (colour: interleaved pixels; 16-bit formats: uint16
        samples in host byte order; Bayer: the mosaic, one sample per pixel — all converted on the device)"""
        self._ck(self.L.rvio_hip_set_image_format(self.h, int(fmt)), "set_image_format")
        bpp, self.sample_dtype, ch = abi.PIX_LAYOUT[int(fmt)]
        self.channels = ch or 1

    def image_format(self):
        return int(self.L.rvio_hip_get_image_format(self.h))

    def _img(self, img):
        """(array, row stride in bytes): a row-strided view of the format's sample type is handed over as it is (cv::Mat::step), anything else is
        packed.  H x W with the mono formats and the Bayer mosaics, H x W x 3|4 (interleaved) with a colour format, uint16 samples with a 16-bit
        format (abi.PIX_LAYOUT): any other shape is refused, and so is an array that is not uint16 handed to a 16-bit format"""
        img = np.asarray(img)
        ch = self.channels
        dt = np.dtype(getattr(self, "sample_dtype", "uint8"))
        if img.ndim != (2 if ch == 1 else 3) or (ch > 1 and img.shape[2] != ch):
            raise RvioHipError("image of shape %s handed to a handle whose format has %d sample(s) per pixel (set_image_format)" % (img.shape, ch))
        if dt == np.uint16 and img.dtype != np.uint16:
            raise RvioHipError("%s image handed to a handle whose format has 16-bit samples (set_image_format)" % img.dtype)
        sz = dt.itemsize
        if ch == 1:
            if img.dtype != dt or img.strides[1] != sz or img.strides[0] < img.shape[1] * sz:
                img = np.ascontiguousarray(img, dt)
        elif img.dtype != dt or img.strides[2] != sz or img.strides[1] != ch * sz or img.strides[0] < img.shape[1] * ch * sz:
            img = np.ascontiguousarray(img, dt)
        return img, img.strides[0]

    def track(self, img, imu, cand=None):
        img, stride = self._img(img)
        imu = np.ascontiguousarray(imu)
        cp, cn, _keep = self._cand(cand)
        self._ck(self.L.rvio_hip_track(self.h, C.cast(img.ctypes.data, up), stride, imu.ctypes.data_as(C.POINTER(abi.rvio_imu)), len(imu),
                                       cp, cn), "track")

    def frame(self, img, imu, cand=None):
        """whole MonoVIO body from host buffers (System.cc:253-367); cand=None: device detector"""
        img, stride = self._img(img)
        imu = np.ascontiguousarray(imu)
        cp, cn, _keep = self._cand(cand)
        self._ck(self.L.rvio_hip_frame(self.h, C.cast(img.ctypes.data, up), stride, imu.ctypes.data_as(C.POINTER(abi.rvio_imu)), len(imu),
                                       cp, cn), "frame")

    def get_corners(self, want_eig=False):
        """last result of the device detector: (refined corners, goodFeaturesToTrack corners[, min-eigenvalue map])"""
        F = self.cfg.n_features
        n = C.c_int32(0)
        xy, raw = np.zeros((F, 2), np.float32), np.zeros((F, 2), np.float32)
        eig = np.zeros((self.cfg.height, self.cfg.width), np.float32) if want_eig else None
        self._ck(self.L.rvio_hip_get_corners(self.h, C.byref(n), _p(xy, fp), _p(raw, fp), _p(eig, fp) if want_eig else None), "get_corners")
        return (xy[: n.value].copy(), raw[: n.value].copy()) + ((eig,) if want_eig else ())

    def track_points(self, tracked, status, imu, cand):
        tracked = np.ascontiguousarray(tracked, np.float32)
        status = np.ascontiguousarray(status, np.uint8)
        imu = np.ascontiguousarray(imu)
        cand = np.ascontiguousarray(cand, np.float32)
        self._ck(self.L.rvio_hip_track_points(self.h, _p(tracked, fp), _p(status, up), len(status),
                                              imu.ctypes.data_as(C.POINTER(abi.rvio_imu)), len(imu), _p(cand, fp), len(cand)), "track_points")

    def frame_points(self, tracked, status, imu, cand):
        tracked = np.ascontiguousarray(tracked, np.float32)
        status = np.ascontiguousarray(status, np.uint8)
        imu = np.ascontiguousarray(imu)
        cand = np.ascontiguousarray(cand, np.float32)
        self._ck(self.L.rvio_hip_frame_points(self.h, _p(tracked, fp), _p(status, up), len(status),
                                              imu.ctypes.data_as(C.POINTER(abi.rvio_imu)), len(imu), _p(cand, fp), len(cand)), "frame_points")

    def frame_dev(self, d_img_ptr, stride, d_imu_ptr, m, d_cand_ptr, n_cand):
        self._ck(self.L.rvio_hip_frame_dev(self.h, C.c_void_p(d_img_ptr), int(stride), C.c_void_p(d_imu_ptr), int(m),
                                           C.c_void_p(d_cand_ptr), int(n_cand)), "frame_dev")

    def track_dev(self, d_img_ptr, stride, d_imu_ptr, m, d_cand_ptr, n_cand):
        self._ck(self.L.rvio_hip_track_dev(self.h, C.c_void_p(d_img_ptr), int(stride), C.c_void_p(d_imu_ptr), int(m),
                                           C.c_void_p(d_cand_ptr), int(n_cand)), "track_dev")

    def frame_plan(self):
        du, da = C.c_int(0), C.c_int(0)
        self._ck(self.L.rvio_hip_frame_plan(self.h, C.byref(du), C.byref(da)), "frame_plan")
        return bool(du.value), bool(da.value)

    def propagate_dev(self, d_imu_ptr, m):
        self._ck(self.L.rvio_hip_propagate_dev(self.h, C.c_void_p(d_imu_ptr), int(m)), "propagate_dev")

    def update_local_tracked(self, rank, world):
        """stage A of the sharded updater on the tracker's device-resident tracks"""
        ptr, n = dp(), C.c_int(0)
        self._ck(self.L.rvio_hip_update_local(self.h, None, rank, world, C.byref(ptr), C.byref(n)), "update_local")
        return C.cast(ptr, C.c_void_p).value, n.value

    def frame_tail_staged(self, d_imu_ptr, m, evs, stream, torch):
        """propagate -> [update] -> augment/compose with events evs[2..4] recorded between the stages"""
        do_update, do_augment = self.frame_plan()
        self.propagate_dev(d_imu_ptr, m)
        with torch.cuda.stream(stream):
            evs[2].record()
        if do_update:
            self.update_tracked()
        with torch.cuda.stream(stream):
            evs[3].record()
        self.augment_compose(do_augment)
        with torch.cuda.stream(stream):
            evs[4].record()
        return do_update

    def frame_begin_dev(self, d_img_ptr, stride, d_imu_ptr, m, d_cand_ptr, n_cand):
        self._ck(self.L.rvio_hip_frame_begin_dev(self.h, C.c_void_p(d_img_ptr), int(stride), C.c_void_p(d_imu_ptr), int(m),
                                                 C.c_void_p(d_cand_ptr), int(n_cand)), "frame_begin_dev")

    def frame_end(self):
        self._ck(self.L.rvio_hip_frame_end(self.h), "frame_end")

    def frame_sharded_dev(self, d_img_ptr, stride, d_imu_ptr, m, d_cand_ptr, n_cand, rank, world, comm=None, allgather=None):
        """one pipelined frame with the feature-sharded updater behind ONE C-ABI call; comm: ncclComm_t (int / c_void_p), None with world 1"""
        cp = comm.value if isinstance(comm, C.c_void_p) else comm
        self._ck(self.L.rvio_hip_frame_sharded_dev(self.h, C.c_void_p(d_img_ptr), int(stride), C.c_void_p(d_imu_ptr), int(m), C.c_void_p(d_cand_ptr), int(n_cand),
                                                   int(rank), int(world), C.c_void_p(cp), C.c_void_p(allgather)), "frame_sharded_dev")

    def frame_sharded_piped(self, d_img_ptr, stride, d_imu_ptr, m, d_cand_ptr, n_cand, rank, world, gathered, dist, DeviceArray, torch, stream,
                            force_collective=False, comm=None):
        """One pipelined frame with the feature-sharded updater, no host synchronisation: the front end of this
        frame overlaps the previous frame's filter work; local [A|b] block -> ONE all-gather, enqueued behind the block kernel
        because the handle's filter stream is torch's current stream -> replicated global update."""
        with torch.cuda.stream(stream):
            self.frame_begin_dev(d_img_ptr, stride, d_imu_ptr, m, d_cand_ptr, n_cand)
            do_update, do_augment = self.frame_plan()
            if do_update:
                if world > 1 or force_collective:
                    ptr, n = self.update_local_tracked(rank, world)
                    if comm is not None:       # RCCL directly on the filter stream (rccl.py): plain stream order, nothing else
                        comm.all_gather_f64(ptr, gathered.data_ptr(), n, self.stream())
                    else:
                        if getattr(self, "_local_key", None) != (ptr, n):  # the block lives in one fixed device buffer: wrap it once
                            self._local_key, self._local = (ptr, n), torch.as_tensor(DeviceArray(ptr, n), device="cuda")
                        dist.all_gather_into_tensor(gathered[: world * n], self._local)     # (the payload grows with the window: n doubles per rank, rank-major)
                    self.update_global(gathered.data_ptr(), world)
                else:
                    self._ck(self.L.rvio_hip_update_tracked(self.h), "update_tracked")
            self.augment_compose(do_augment)
            self.frame_end()

    def frame_tail_sharded(self, d_imu_ptr, m, rank, world, gathered, dist, DeviceArray, torch):
        """Feature-sharded frame tail: local [A|b] block -> ONE all-gather -> replicated EKF update."""
        do_update, do_augment = self.frame_plan()
        self.propagate_dev(d_imu_ptr, m)
        if do_update:
            ptr, n = self.update_local_tracked(rank, world)
            self.sync()                                   # block ready (handle stream) before the collective's stream reads it
            local = torch.as_tensor(DeviceArray(ptr, n), device="cuda")
            dist.all_gather_into_tensor(gathered[: world * n], local)
            torch.cuda.current_stream().synchronize()     # gathered blocks visible before the handle stream consumes them
            self.update_global(gathered.data_ptr(), world)
        self.augment_compose(do_augment)

    def get_tracks(self):
        ML = self.cfg.max_track_len
        types, lens, meas = np.zeros(self.Fu, np.uint8), np.zeros(self.Fu, np.int32), np.zeros((self.Fu, ML, 2), np.float32)
        n = C.c_int32(0)
        self._ck(self.L.rvio_hip_get_tracks(self.h, C.byref(n), _p(types, up), _p(lens, ip), _p(meas, fp)), "get_tracks")
        return types[: n.value].copy(), lens[: n.value].copy(), meas[: n.value].copy()

    def get_points_at(self, i):
        F = self.cfg.n_features
        xy, hl = np.zeros((F, 2), np.float32), np.zeros(F, np.int32)
        n = C.c_int32(0)
        self._ck(self.L.rvio_hip_get_tracker_points_at(self.h, int(i), C.byref(n), _p(xy, fp), _p(hl, ip)), "get_tracker_points_at")
        return xy[: n.value].copy(), hl[: n.value].copy()

    def get_points(self):
        F = self.cfg.n_features
        xy, hl = np.zeros((F, 2), np.float32), np.zeros(F, np.int32)
        n = C.c_int32(0)
        self._ck(self.L.rvio_hip_get_tracker_points(self.h, C.byref(n), _p(xy, fp), _p(hl, ip)), "get_tracker_points")
        return xy[: n.value].copy(), hl[: n.value].copy()

    def debug_pyramid(self, level):
        w, hh = C.c_int32(0), C.c_int32(0)
        self._ck(self.L.rvio_hip_debug_pyramid(self.h, level, C.byref(w), C.byref(hh), None, None), "debug_pyramid")
        img = np.zeros((hh.value, w.value), np.uint8)
        dxy = np.zeros((hh.value, w.value, 2), np.int16)
        self._ck(self.L.rvio_hip_debug_pyramid(self.h, level, C.byref(w), C.byref(hh), _p(img, up),
                                               dxy.ctypes.data_as(C.POINTER(C.c_int16))), "debug_pyramid")
        return img, dxy

    def debug_tracked(self, n):
        xy, un = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        self._ck(self.L.rvio_hip_debug_tracked(self.h, n, _p(xy, fp), _p(un, fp)), "debug_tracked")
        return xy, un

    def time_kernel(self, which, iters=20):
        """average device time (us) of one hot kernel: 0 solve, 1 KLT, 2 per-feature build, 3 share reduction, 4 U/G/P1, 5 Joseph form, 6 cornerSubPix, 7 U/G/P1 + Joseph form as launched, 8 feat_prop_kernel as the pipelined frame launches it (state restored), 9 the detector's greedy selection, 10 the landmark cloud kernel, 11 the gray conversion of the last colour or raw (16-bit, Bayer) image in the form the frame launched, 12 the odometry record kernel, 13 the IMU-pose kernel on the state and IMU batch of the last frame, 14 the IMU-covariance kernel on the same operands, 15 the landmark-covariance kernel on the last update's cloud and operands (HIP events, handle stream)"""
        us = C.c_float(0)
        self._ck(self.L.rvio_hip_debug_time_kernel(self.h, int(which), int(iters), C.byref(us)), "debug_time_kernel")
        return float(us.value)

    def poison(self, what=7):
        """drain the handle, then overwrite left-over state: 1 filter scratch, 2 LDS of the chip, 4 hand-over tables + tracker scratch + gray buffers, 8 set error bit 4"""
        self._ck(self.L.rvio_hip_debug_poison(self.h, int(what)), "debug_poison")

    def stall(self, which, usec):
        """occupy one of the handle's streams (0 filter, 1 tracker / image chain 0, 2 side, 3 image chain 1) for usec microseconds"""
        self._ck(self.L.rvio_hip_debug_stall(self.h, int(which), int(usec)), "debug_stall")

    def noise(self, wgs, usec):
        """`wgs` workgroups of HBM / L2 / LDS traffic on a stream of their own for usec microseconds (a box under load)"""
        self._ck(self.L.rvio_hip_debug_noise(self.h, int(wgs), int(usec)), "debug_noise")

    def kernel_forms(self, throughput):
        """select the throughput (batch) or latency (one stream) forms of the image kernels on this handle: same bits either way"""
        self._ck(self.L.rvio_hip_debug_kernel_forms(self.h, int(throughput)), "debug_kernel_forms")

    def frame_info(self):
        info = abi.rvio_frame_info()
        self._ck(self.L.rvio_hip_get_frame_info(self.h, C.byref(info)), "get_frame_info")
        return info.asdict()

    def pose(self):
        p, q = np.zeros(3), np.zeros(4)
        self._ck(self.L.rvio_hip_get_pose(self.h, _p(p, dp), _p(q, dp)), "get_pose")
        return p, q

    get_pose = pose

    def get_pose_at(self, i):
        """pose line (pGk, qkG) of instance i of a batch handle"""
        p, q = np.zeros(3), np.zeros(4)
        self._ck(self.L.rvio_hip_get_pose_at(self.h, int(i), _p(p, dp), _p(q, dp)), "get_pose_at")
        return p, q

    # ---- odometry ring (System.cc:402-434)
    def set_odometry(self, capacity):
        """keep an rvio_odom record of every frame from the next augment/compose stage on, `capacity` per instance on the device; 0: off"""
        self._ck(self.L.rvio_hip_set_odometry(self.h, int(capacity)), "set_odometry")
        if capacity:
            self._odom_cap = int(capacity)

    def odometry(self, instance=0, first_seq=1, max_n=None):
        """records of one instance still in the ring with seq >= first_seq, oldest first (at most max_n): a structured array (abi.ODOM_DTYPE)"""
        cap = getattr(self, "_odom_cap", 0) if max_n is None else int(max_n)
        out = np.zeros(max(cap, 0), abi.ODOM_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.rvio_hip_get_odometry(self.h, int(instance), C.c_int64(int(first_seq)), cap,
                                              out.ctypes.data_as(C.POINTER(abi.rvio_odom)) if len(out) else None, C.byref(n)), "get_odometry")
        return out[: n.value].copy()

    def odometry_all(self):
        """(seq, the newest record of every instance); seq = 0 and zeroed records before the first frame"""
        out = np.zeros(self.batch, abi.ODOM_DTYPE)
        seq = C.c_int64(0)
        self._ck(self.L.rvio_hip_get_odometry_all(self.h, out.ctypes.data_as(C.POINTER(abi.rvio_odom)), C.byref(seq)), "get_odometry_all")
        return int(seq.value), out

    # ---- fixed-lag smoothed trajectory (csrc/window_pose.hip)
    def get_window(self, instance=0, max_n=None):
        """pose and covariance of the frames of ages 0 .. min(n_clones, max_n - 1) of one instance, newest first, at the state as it is now
        (abi.WINDOW_POSE_DTYPE)"""
        cap = self.nmax + 1 if max_n is None else int(max_n)
        out = np.zeros(max(cap, 1), abi.WINDOW_POSE_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.rvio_hip_get_window(self.h, int(instance), cap, out.ctypes.data_as(C.POINTER(abi.rvio_window_pose)), C.byref(n)), "get_window")
        return out[: n.value].copy()

    def get_window_dev(self, age_first, n_ages, d_out_ptr, out_stride):
        """every instance, ages age_first .. age_first + n_ages - 1, into device records: (instance, age) at d_out[instance * out_stride + age -
        age_first].  Asynchronous on the filter stream."""
        self._ck(self.L.rvio_hip_get_window_dev(self.h, int(age_first), int(n_ages), C.c_void_p(d_out_ptr), C.c_size_t(int(out_stride))), "get_window_dev")

    def set_smoothed_odometry(self, capacity, lag):
        """keep an rvio_window_pose record of the frame `lag` images back behind every augment/compose stage from the next one on, `capacity` per
        instance on the device; 0: off"""
        self._ck(self.L.rvio_hip_set_smoothed_odometry(self.h, int(capacity), int(lag)), "set_smoothed_odometry")
        if capacity:
            self._smo_cap = int(capacity)

    def smoothed_odometry(self, instance=0, first_seq=1, max_n=None):
        """records of one instance still in the smoothed ring with seq >= first_seq, oldest first (at most max_n): abi.WINDOW_POSE_DTYPE"""
        cap = getattr(self, "_smo_cap", 0) if max_n is None else int(max_n)
        out = np.zeros(max(cap, 0), abi.WINDOW_POSE_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.rvio_hip_get_smoothed_odometry(self.h, int(instance), C.c_int64(int(first_seq)), cap,
                                                       out.ctypes.data_as(C.POINTER(abi.rvio_window_pose)) if len(out) else None, C.byref(n)), "get_smoothed_odometry")
        return out[: n.value].copy()

    def smoothed_odometry_all(self):
        """(seq, the newest smoothed record of every instance); seq = 0 and zeroed records before the first one"""
        out = np.zeros(self.batch, abi.WINDOW_POSE_DTYPE)
        seq = C.c_int64(0)
        self._ck(self.L.rvio_hip_get_smoothed_odometry_all(self.h, out.ctypes.data_as(C.POINTER(abi.rvio_window_pose)), C.byref(seq)), "get_smoothed_odometry_all")
        return int(seq.value), out

    # ---- pose-graph export: window edges and the joint covariance of the window's poses (csrc/window_edge.hip)
    def get_window_edges(self, pairs, instance=0):
        """the edges (relative pose and its covariance) between the frames (age_new, age_old) of `pairs` of one instance, at the state as it is
        now (abi.WINDOW_EDGE_DTYPE)"""
        pr = np.asarray(pairs, np.int32).reshape(-1, 2)
        a, b = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        out = np.zeros(max(len(pr), 1), abi.WINDOW_EDGE_DTYPE)
        self._ck(self.L.rvio_hip_get_window_edges(self.h, int(instance), len(pr), a.ctypes.data_as(C.POINTER(C.c_int32)), b.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  out.ctypes.data_as(C.POINTER(abi.rvio_window_edge))), "get_window_edges")
        return out[: len(pr)].copy()

    def get_window_edges_dev(self, n_pairs, d_age_new_ptr, d_age_old_ptr, d_out_ptr, out_stride):
        """every instance, one pair list on the device for all of them: (instance, pair) at d_out[instance * out_stride + pair].  Asynchronous on
        the filter stream."""
        self._ck(self.L.rvio_hip_get_window_edges_dev(self.h, int(n_pairs), C.c_void_p(d_age_new_ptr), C.c_void_p(d_age_old_ptr), C.c_void_p(d_out_ptr),
                                                      C.c_size_t(int(out_stride))), "get_window_edges_dev")

    def set_edge_odometry(self, capacity, age_new, age_old):
        """keep an rvio_window_edge record of the pair (age_new, age_old) behind every augment/compose stage from the next one on, `capacity` per
        instance on the device; 0: off"""
        self._ck(self.L.rvio_hip_set_edge_odometry(self.h, int(capacity), int(age_new), int(age_old)), "set_edge_odometry")
        if capacity:
            self._edg_cap = int(capacity)

    def edge_odometry(self, instance=0, first_seq=1, max_n=None):
        """records of one instance still in the edge ring with seq >= first_seq, oldest first (at most max_n): abi.WINDOW_EDGE_DTYPE"""
        cap = getattr(self, "_edg_cap", 0) if max_n is None else int(max_n)
        out = np.zeros(max(cap, 0), abi.WINDOW_EDGE_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.rvio_hip_get_edge_odometry(self.h, int(instance), C.c_int64(int(first_seq)), cap,
                                                   out.ctypes.data_as(C.POINTER(abi.rvio_window_edge)) if len(out) else None, C.byref(n)), "get_edge_odometry")
        return out[: n.value].copy()

    def edge_odometry_all(self):
        """(seq, the newest edge record of every instance); seq = 0 and zeroed records before the first one"""
        out = np.zeros(self.batch, abi.WINDOW_EDGE_DTYPE)
        seq = C.c_int64(0)
        self._ck(self.L.rvio_hip_get_edge_odometry_all(self.h, out.ctypes.data_as(C.POINTER(abi.rvio_window_edge)), C.byref(seq)), "get_edge_odometry_all")
        return int(seq.value), out

    def get_window_joint(self, instance=0, max_n=None):
        """(poses, cov): the rvio_window_pose records of ages 0 .. m - 1, m = min(n_clones + 1, max_n), newest first, and the joint covariance
        (6 m x 6 m) of those poses, block (a, b) = J_a P J_b^T"""
        cap = self.nmax + 1 if max_n is None else int(max_n)
        poses = np.zeros(max(cap, 1), abi.WINDOW_POSE_DTYPE)
        cov = np.zeros((6 * max(cap, 1), 6 * max(cap, 1)))
        n = C.c_int32(0)
        self._ck(self.L.rvio_hip_get_window_joint(self.h, int(instance), cap, poses.ctypes.data_as(C.POINTER(abi.rvio_window_pose)),
                                                  cov.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(cov.shape[1]), C.byref(n)), "get_window_joint")
        m = n.value
        return poses[:m].copy(), cov[: 6 * m, : 6 * m].copy()

    def get_window_joint_dev(self, n_ages, d_poses_ptr, pose_stride, d_cov_ptr, cov_stride):
        """every instance, ages 0 .. n_ages - 1: pose (instance, age) at d_poses[instance * pose_stride + age], the instance's 6 n_ages x 6 n_ages
        matrix at d_cov + instance * cov_stride doubles.  Asynchronous on the filter stream."""
        self._ck(self.L.rvio_hip_get_window_joint_dev(self.h, int(n_ages), C.c_void_p(d_poses_ptr), C.c_size_t(int(pose_stride)), C.c_void_p(d_cov_ptr),
                                                      C.c_size_t(int(cov_stride))), "get_window_joint_dev")

    # ---- IMU-rate odometry (PreIntegrator.cc:168-176 kept per sample)
    def predict(self, imu, instance=0):
        """dead reckoning: the pose behind every sample of `imu` from the CURRENT state of one instance (abi.IMU_POSE_DTYPE); mutates nothing"""
        imu = np.ascontiguousarray(imu)
        out = np.zeros(len(imu), abi.IMU_POSE_DTYPE)
        self._ck(self.L.rvio_hip_predict(self.h, int(instance), imu.ctypes.data_as(C.POINTER(abi.rvio_imu)) if len(imu) else None, len(imu),
                                         out.ctypes.data_as(C.POINTER(abi.ImuPose)) if len(out) else None), "predict")
        return out

    def predict_dev(self, d_imu_ptr, imu_stride, m, d_out_ptr, out_stride):
        """the same for every instance, device buffers, asynchronous on the filter stream: d_out[z * out_stride + j]"""
        self._ck(self.L.rvio_hip_predict_dev(self.h, C.c_void_p(d_imu_ptr), int(imu_stride), int(m), C.c_void_p(d_out_ptr), int(out_stride)), "predict_dev")

    def set_imu_odometry(self, capacity):
        """keep an rvio_imu_pose record of every IMU sample any propagate consumes from now on, `capacity` per instance on the device; 0: off"""
        self._ck(self.L.rvio_hip_set_imu_odometry(self.h, int(capacity)), "set_imu_odometry")
        if capacity:
            self._imuo_cap = int(capacity)

    def get_imu_odometry(self, instance=0, first_seq=1, max_n=None):
        """records of one instance still in the IMU-rate ring with seq >= first_seq, oldest first (at most max_n): abi.IMU_POSE_DTYPE"""
        cap = getattr(self, "_imuo_cap", 0) if max_n is None else int(max_n)
        out = np.zeros(max(cap, 0), abi.IMU_POSE_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.rvio_hip_get_imu_odometry(self.h, int(instance), C.c_int64(int(first_seq)), cap,
                                                  out.ctypes.data_as(C.POINTER(abi.ImuPose)) if len(out) else None, C.byref(n)), "get_imu_odometry")
        return out[: n.value].copy()

    # ---- IMU-rate odometry with covariance (PreIntegrator.cc:123-142 kept per sample, composed as System.cc:325-365)
    def predict_cov(self, imu, instance=0, poses=True):
        """predict plus the covariance record of every sample: (abi.IMU_POSE_DTYPE records or None, abi.IMU_COV_DTYPE records); mutates nothing"""
        imu = np.ascontiguousarray(imu)
        out = np.zeros(len(imu), abi.IMU_POSE_DTYPE) if poses else None
        cov = np.zeros(len(imu), abi.IMU_COV_DTYPE)
        self._ck(self.L.rvio_hip_predict_cov(self.h, int(instance), imu.ctypes.data_as(C.POINTER(abi.rvio_imu)) if len(imu) else None, len(imu),
                                             out.ctypes.data_as(C.POINTER(abi.ImuPose)) if poses and len(imu) else None,
                                             cov.ctypes.data_as(C.POINTER(abi.ImuCov)) if len(cov) else None), "predict_cov")
        return out, cov

    def predict_cov_dev(self, d_imu_ptr, imu_stride, m, d_out_ptr, out_stride, d_cov_ptr, cov_stride):
        """the same for every instance, device buffers, asynchronous on the filter stream: d_cov[z * cov_stride + j]; d_out_ptr None / 0: covariances only"""
        self._ck(self.L.rvio_hip_predict_cov_dev(self.h, C.c_void_p(d_imu_ptr), int(imu_stride), int(m), C.c_void_p(d_out_ptr) if d_out_ptr else None, int(out_stride),
                                                 C.c_void_p(d_cov_ptr), int(cov_stride)), "predict_cov_dev")

    def set_imu_odometry_cov(self, enable):
        """keep an rvio_imu_cov record beside every record of the IMU-rate ring from now on (that ring's capacity, seq and slots); 0: off"""
        self._ck(self.L.rvio_hip_set_imu_odometry_cov(self.h, int(enable)), "set_imu_odometry_cov")

    def get_imu_odometry_cov(self, instance=0, first_seq=1, max_n=None):
        """covariance records of one instance still in the ring with seq >= first_seq, oldest first (at most max_n): abi.IMU_COV_DTYPE"""
        cap = getattr(self, "_imuo_cap", 0) if max_n is None else int(max_n)
        out = np.zeros(max(cap, 0), abi.IMU_COV_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.rvio_hip_get_imu_odometry_cov(self.h, int(instance), C.c_int64(int(first_seq)), cap,
                                                      out.ctypes.data_as(C.POINTER(abi.ImuCov)) if len(out) else None, C.byref(n)), "get_imu_odometry_cov")
        return out[: n.value].copy()

    # ---- auxiliary measurement update (Updater.cc:540-619 with a full-width H)
    def update_aux(self, H, v, sigma, mode=abi.RVIO_AUX_RESIDUAL, gate=0, instance=-1):
        """fuse m <= 16 rows (H: m x d in the error-state order of P, R = diag(sigma^2)) into (x, P) in place on the device; mode VALUE: v is the
        measured value and the device forms v - H xi(x); gate: apply iff gamma < chi2_95(m); instance -1: every instance.  Asynchronous."""
        ms = abi.make_aux_meas(H, v, sigma, mode, gate)
        self._ck(self.L.rvio_hip_update_aux(self.h, int(instance), C.byref(ms)), "update_aux")

    def update_aux_dev(self, m, mode, gate, d_H_ptr, H_stride, d_v_ptr, v_stride, d_sigma_ptr, sigma_stride, d_active_ptr=None):
        """the same on device buffers for every instance in one launch (strides in doubles, 0: shared; d_active: B int32 flags or None)"""
        self._ck(self.L.rvio_hip_update_aux_dev(self.h, int(m), int(mode), int(gate), C.c_void_p(d_H_ptr), C.c_size_t(int(H_stride)), C.c_void_p(d_v_ptr),
                                                C.c_size_t(int(v_stride)), C.c_void_p(d_sigma_ptr), C.c_size_t(int(sigma_stride)),
                                                C.c_void_p(d_active_ptr) if d_active_ptr else None), "update_aux_dev")

    def aux_diag(self, instance=0):
        """(gamma, applied) of one instance in the last update_aux* call"""
        g, a = C.c_double(0), C.c_int32(0)
        self._ck(self.L.rvio_hip_get_aux_diag(self.h, int(instance), C.byref(g), C.byref(a)), "get_aux_diag")
        return float(g.value), int(a.value)

    # ---- standstill detection and the automatic zero-velocity update (csrc/standstill.hip in front of the auxiliary update)
    def set_standstill(self, c):
        """switch the feature on with an abi.rvio_standstill_config, off with None"""
        self._ck(self.L.rvio_hip_set_standstill(self.h, C.byref(c) if c is not None else None), "set_standstill")

    def standstill(self, imu, apply=1):
        """one decision per instance from the IMU batch (host records, shared by every instance); apply: fuse zero velocity into the static ones.  Asynchronous."""
        imu = np.ascontiguousarray(imu)
        self._ck(self.L.rvio_hip_standstill(self.h, imu.ctypes.data_as(C.POINTER(abi.rvio_imu)) if len(imu) else None, len(imu), int(apply)), "standstill")

    def standstill_dev(self, d_imu_ptr, imu_stride, m, apply=1):
        """the same on a device buffer: instance z reads d_imu + z * imu_stride (0: shared)"""
        self._ck(self.L.rvio_hip_standstill_dev(self.h, C.c_void_p(d_imu_ptr), int(imu_stride), int(m), int(apply)), "standstill_dev")

    def get_standstill(self, instance=0):
        """the abi.rvio_standstill record of one instance from the last standstill* call (waits for the filter stream only)"""
        r = abi.rvio_standstill()
        self._ck(self.L.rvio_hip_get_standstill(self.h, int(instance), C.byref(r)), "get_standstill")
        return r

    # ---- absolute fixes: position, attitude, pose, gravity rows linearised on the device (csrc/fix_rows.hip in front of the auxiliary update)
    def update_fix(self, kind, fix, gate=0, instance=-1):
        """fuse one abi.rvio_fix (host record) of kind abi.RVIO_FIX_*; instance: 0 .. B - 1, or -1 = every instance.  Asynchronous."""
        self._ck(self.L.rvio_hip_update_fix(self.h, int(instance), int(kind), int(gate), C.byref(fix) if fix is not None else None), "update_fix")

    def update_fix_dev(self, kind, gate, d_fix_ptr, fix_stride=0, d_active_ptr=None):
        """the same on device records: instance z reads d_fix + z * fix_stride records (0: shared); d_active: None or one int32 per instance"""
        self._ck(self.L.rvio_hip_update_fix_dev(self.h, int(kind), int(gate), C.c_void_p(d_fix_ptr), C.c_size_t(int(fix_stride)),
                                                C.c_void_p(d_active_ptr) if d_active_ptr else None), "update_fix_dev")

    def get_fix(self, instance=0):
        """the abi.rvio_fix_diag record of one instance from the last update_fix* call (waits for the filter stream only)"""
        r = abi.rvio_fix_diag()
        self._ck(self.L.rvio_hip_get_fix(self.h, int(instance), C.byref(r)), "get_fix")
        return r

    def get_fix_rows(self, instance=0):
        """(H [m x d], sigma [m]) as the device formed them in the last update_fix* call"""
        m, d = C.c_int32(0), C.c_int32(0)
        self._ck(self.L.rvio_hip_get_fix_rows(self.h, int(instance), C.byref(m), C.byref(d), None, None), "get_fix_rows")
        H, sigma = np.zeros((m.value, d.value)), np.zeros(m.value)
        dp = C.POINTER(C.c_double)
        self._ck(self.L.rvio_hip_get_fix_rows(self.h, int(instance), C.byref(m), C.byref(d), H.ctypes.data_as(dp), sigma.ctypes.data_as(dp)), "get_fix_rows")
        return H, sigma


    # ---- past-frame fixes: a delayed fix linearised against the frame it was taken at (csrc/fix_past.hip in front of the auxiliary update)
    def update_fix_past(self, kind, fix, age, frac=0.0, gate=0, instance=-1):
        """fuse one abi.rvio_fix (host record) taken `age` images back from the newest composed frame (POSITION: frac of the way towards
        age + 1); instance: 0 .. B - 1, or -1 = every instance.  Asynchronous."""
        self._ck(self.L.rvio_hip_update_fix_past(self.h, int(instance), int(kind), int(gate), int(age), C.c_double(float(frac)),
                                                 C.byref(fix) if fix is not None else None), "update_fix_past")

    def update_fix_past_dev(self, kind, gate, d_fix_ptr, fix_stride, d_age_ptr, d_frac_ptr=None, d_active_ptr=None):
        """the same on device records: d_age one int32 per instance, d_frac None (0) or one double per instance"""
        self._ck(self.L.rvio_hip_update_fix_past_dev(self.h, int(kind), int(gate), C.c_void_p(d_fix_ptr), C.c_size_t(int(fix_stride)), C.c_void_p(d_age_ptr),
                                                     C.c_void_p(d_frac_ptr) if d_frac_ptr else None, C.c_void_p(d_active_ptr) if d_active_ptr else None),
                 "update_fix_past_dev")

    def frame_age(self, img_count):
        """the age the frame counted img_count has now (host arithmetic only); raises when it is not composed yet or has left the window"""
        a = C.c_int(0)
        self._ck(self.L.rvio_hip_frame_age(self.h, int(img_count), C.byref(a)), "frame_age")
        return a.value

    # ---- relative-pose measurements between two frames of the window (csrc/rel_rows.hip in front of the auxiliary update)
    def update_rel(self, kind, meas, age_new, age_old, gate=0, instance=-1):
        """fuse one abi.rvio_fix (host record) of kind abi.RVIO_REL_*: the delta pose between the frames age_old and age_new < age_old images
        back from the newest composed frame; instance: 0 .. B - 1, or -1 = every instance.  Asynchronous."""
        self._ck(self.L.rvio_hip_update_rel(self.h, int(instance), int(kind), int(gate), int(age_new), int(age_old),
                                            C.byref(meas) if meas is not None else None), "update_rel")

    def update_rel_dev(self, kind, gate, d_meas_ptr, meas_stride, d_age_new_ptr, d_age_old_ptr, d_active_ptr=None):
        """the same on device records: d_age_new / d_age_old one int32 per instance"""
        self._ck(self.L.rvio_hip_update_rel_dev(self.h, int(kind), int(gate), C.c_void_p(d_meas_ptr), C.c_size_t(int(meas_stride)), C.c_void_p(d_age_new_ptr),
                                                C.c_void_p(d_age_old_ptr), C.c_void_p(d_active_ptr) if d_active_ptr else None), "update_rel_dev")

    # ---- map landmarks: pixel observations of known world points (csrc/map_rows.hip in front of the auxiliary update)
    def update_map(self, obs, age, units=abi.RVIO_MAP_NORMALISED, gate=0, gate_each=1, instance=-1):
        """fuse 1 .. 8 abi.rvio_map_obs (a ctypes array, abi.make_map_obs) made in the image `age` back from the newest composed frame; gate_each:
        the chi-square gate per point; gate: the stack gate; instance: 0 .. B - 1, or -1 = every instance.  Asynchronous."""
        self._ck(self.L.rvio_hip_update_map(self.h, int(instance), int(units), int(gate), int(gate_each), int(age), len(obs) if obs is not None else 0,
                                            obs if obs is not None else None), "update_map")

    def update_map_dev(self, units, gate, gate_each, n_max, d_obs_ptr, obs_stride, d_count_ptr, d_age_ptr, d_active_ptr=None):
        """the same on device records: instance z reads d_obs + z * obs_stride records (0: shared), d_count[z] of them (None: n_max each) at the
        age d_age[z]"""
        self._ck(self.L.rvio_hip_update_map_dev(self.h, int(units), int(gate), int(gate_each), int(n_max), C.c_void_p(d_obs_ptr), C.c_size_t(int(obs_stride)),
                                                C.c_void_p(d_count_ptr) if d_count_ptr else None, C.c_void_p(d_age_ptr) if d_age_ptr else None,
                                                C.c_void_p(d_active_ptr) if d_active_ptr else None), "update_map_dev")

    def get_map(self, instance=0):
        """(abi.rvio_map_diag, [8 abi.rvio_map_point]) of one instance from the last update_map* call (waits for the filter stream only)"""
        rec, pts = abi.rvio_map_diag(), (abi.rvio_map_point * abi.RVIO_MAP_MAX_POINTS)()
        self._ck(self.L.rvio_hip_get_map(self.h, int(instance), C.byref(rec), pts), "get_map")
        return rec, list(pts)

    def get_map_rows(self, instance=0):
        """(H [m x d], r [m], sigma [m]) as the device formed them in the last update_map* call"""
        m, d = C.c_int32(0), C.c_int32(0)
        self._ck(self.L.rvio_hip_get_map_rows(self.h, int(instance), C.byref(m), C.byref(d), None, None, None), "get_map_rows")
        H, r, sigma = np.zeros((m.value, d.value)), np.zeros(m.value), np.zeros(m.value)
        dp = C.POINTER(C.c_double)
        self._ck(self.L.rvio_hip_get_map_rows(self.h, int(instance), C.byref(m), C.byref(d), H.ctypes.data_as(dp), r.ctypes.data_as(dp), sigma.ctypes.data_as(dp)),
                 "get_map_rows")
        return H, r, sigma

    # ---- iterated measurement updates: the fix, past-fix, rel and map calls relinearised max_iters times on the device
    def set_meas_iterations(self, max_iters, tol=0.0):
        """a handle setting: 1 .. abi.RVIO_MEAS_MAX_ITERS passes, an instance finished once max |dx_new - dx| < tol (0: always max_iters passes);
        1 (the default) is the plain update"""
        self._ck(self.L.rvio_hip_set_meas_iterations(self.h, int(max_iters), C.c_double(float(tol))), "set_meas_iterations")

    def get_meas_iterations(self):
        """(max_iters, tol) as set"""
        k, t = C.c_int(0), C.c_double(0)
        self._ck(self.L.rvio_hip_get_meas_iterations(self.h, C.byref(k), C.byref(t)), "get_meas_iterations")
        return int(k.value), float(t.value)

    def get_meas_iter(self, instance=0):
        """the abi.rvio_meas_iter record of one instance from the last fix / past-fix / rel / map call (waits for the filter stream only)"""
        r = abi.rvio_meas_iter()
        self._ck(self.L.rvio_hip_get_meas_iter(self.h, int(instance), C.byref(r)), "get_meas_iter")
        return r
