"""ctypes mirror of include/rvio_hip.h (POD structs + function prototypes).

The C header is the source of truth; tests/test_abi.py checks sizeof/offsets
against the compiled library and that every declared symbol is exported.
"""
import ctypes as C
import math
import numpy as np

ABI_VERSION = 6

# rvio_pixel_format (rvio_hip_set_image_format): what the image entry points are handed
RVIO_PIX_MONO8, RVIO_PIX_RGB8, RVIO_PIX_BGR8, RVIO_PIX_RGBA8, RVIO_PIX_BGRA8 = 0, 1, 2, 3, 4
PIX_CHANNELS = {RVIO_PIX_MONO8: 1, RVIO_PIX_RGB8: 3, RVIO_PIX_BGR8: 3, RVIO_PIX_RGBA8: 4, RVIO_PIX_BGRA8: 4}
# raw sensor data (within ABI 6): bit 4 = 16-bit samples (host byte order), bit 5 = a Bayer mosaic named by its top-left 2 x 2 block
RVIO_PIX_MONO16, RVIO_PIX_RGB16, RVIO_PIX_BGR16, RVIO_PIX_RGBA16, RVIO_PIX_BGRA16 = 16, 17, 18, 19, 20
RVIO_PIX_BAYER_RGGB8, RVIO_PIX_BAYER_BGGR8, RVIO_PIX_BAYER_GBRG8, RVIO_PIX_BAYER_GRBG8 = 32, 33, 34, 35
RVIO_PIX_BAYER_RGGB16, RVIO_PIX_BAYER_BGGR16, RVIO_PIX_BAYER_GBRG16, RVIO_PIX_BAYER_GRBG16 = 48, 49, 50, 51
# every format: (bytes per pixel as staged, dtype of the array handed over, trailing dimension of that array or None for H x W)
PIX_LAYOUT = {RVIO_PIX_MONO8: (1, "uint8", None), RVIO_PIX_RGB8: (3, "uint8", 3), RVIO_PIX_BGR8: (3, "uint8", 3),
              RVIO_PIX_RGBA8: (4, "uint8", 4), RVIO_PIX_BGRA8: (4, "uint8", 4),
              RVIO_PIX_MONO16: (2, "uint16", None), RVIO_PIX_RGB16: (6, "uint16", 3), RVIO_PIX_BGR16: (6, "uint16", 3),
              RVIO_PIX_RGBA16: (8, "uint16", 4), RVIO_PIX_BGRA16: (8, "uint16", 4)}
PIX_LAYOUT.update({f: (1, "uint8", None) for f in (32, 33, 34, 35)})
PIX_LAYOUT.update({f: (2, "uint16", None) for f in (48, 49, 50, 51)})
# the names cv_bridge / sensor_msgs give the encodings
PIX_ENCODING = {"mono8": 0, "rgb8": 1, "bgr8": 2, "rgba8": 3, "bgra8": 4, "mono16": 16, "rgb16": 17, "bgr16": 18, "rgba16": 19, "bgra16": 20,
                "bayer_rggb8": 32, "bayer_bggr8": 33, "bayer_gbrg8": 34, "bayer_grbg8": 35,
                "bayer_rggb16": 48, "bayer_bggr16": 49, "bayer_gbrg16": 50, "bayer_grbg16": 51}


class rvio_config(C.Structure):
    _fields_ = [
        ("imu_rate", C.c_double), ("sigma_g", C.c_double), ("sigma_wg", C.c_double),
        ("sigma_a", C.c_double), ("sigma_wa", C.c_double), ("gravity", C.c_double),
        ("small_angle", C.c_double),
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("k1", C.c_float), ("k2", C.c_float), ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float),
        ("sigma_px", C.c_float), ("sigma_py", C.c_float),
        ("T_bc", C.c_double * 16),
        ("fisheye", C.c_int32),
        ("n_features", C.c_int32), ("max_track_len", C.c_int32), ("min_track_len", C.c_int32),
        ("min_dist", C.c_float), ("qual_lvl", C.c_float),
        ("block_x", C.c_float), ("block_y", C.c_float),
        ("enable_equalizer", C.c_int32), ("use_sampson", C.c_int32),
        ("inlier_thr", C.c_double),
        ("ini_thr_angle", C.c_double), ("ini_thr_displ", C.c_double),
        ("ini_enable_alignment", C.c_int32), ("reserved0", C.c_int32),
    ]


class rvio_calibration(C.Structure):
    """what differs between two physical cameras (rvio_hip_set_calibration_at): 168 bytes, no padding"""
    _fields_ = [
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("k1", C.c_float), ("k2", C.c_float), ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float),
        ("fisheye", C.c_int32),
        ("T_bc", C.c_double * 16),
    ]


assert C.sizeof(rvio_calibration) == 168


def calibration_from_config(cfg):
    """the calibration members of an rvio_config (same as C rvio_calibration_from_config)"""
    k = rvio_calibration()
    for name, _ in rvio_calibration._fields_:
        if name != "T_bc":
            setattr(k, name, getattr(cfg, name))
    for i in range(16):
        k.T_bc[i] = cfg.T_bc[i]
    return k


class rvio_imu(C.Structure):
    _fields_ = [("w", C.c_double * 3), ("a", C.c_double * 3), ("t", C.c_double), ("dt", C.c_double)]


IMU_DTYPE = np.dtype([("w", "f8", 3), ("a", "f8", 3), ("t", "f8"), ("dt", "f8")])
assert IMU_DTYPE.itemsize == C.sizeof(rvio_imu) == 64


class rvio_tracks(C.Structure):
    _fields_ = [("n_feat", C.c_int32), ("max_len", C.c_int32),
                ("types", C.POINTER(C.c_ubyte)), ("len", C.POINTER(C.c_int32)), ("meas", C.POINTER(C.c_float))]


class rvio_frame_info(C.Structure):
    _fields_ = [(k, C.c_int32) for k in
                ("n_clones", "n_tracked_in", "n_klt_ok", "n_ransac_inliers", "n_feat_update",
                 "n_feat_accepted", "n_rows", "updated", "n_tracked_out", "ransac_winner")] + \
               [("reserved", C.c_int32 * 5), ("rank_truncated_at", C.c_int32)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        if hasattr(self, "reserved"):
            d["device_error"] = int(self.reserved[0])   # sticky: 1 singular pivot, 2 track the window cannot hold, 4 a device-side stage counter timed out, 8 indefinite gate matrix
            d["literal_rank"] = int(self.reserved[1])   # nRank of the reference's literal Givens sweep + scan when the device ran it for this update (csrc/literal.h), -1 otherwise
        return d


class rvio_odom(C.Structure):
    _fields_ = [("seq", C.c_int64), ("img_count", C.c_int32), ("n_clones", C.c_int32), ("reserved", C.c_int32 * 2),
                ("p", C.c_double * 3), ("q", C.c_double * 4), ("v", C.c_double * 3), ("pose_cov", C.c_double * 36), ("vel_cov", C.c_double * 9)]


ODOM_DTYPE = np.dtype([("seq", "i8"), ("img_count", "i4"), ("n_clones", "i4"), ("reserved", "i4", 2),
                       ("p", "f8", 3), ("q", "f8", 4), ("v", "f8", 3), ("pose_cov", "f8", (6, 6)), ("vel_cov", "f8", (3, 3))])
assert ODOM_DTYPE.itemsize == C.sizeof(rvio_odom) == 464


def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def quat_to_rot(q):
    """QuatToRot (util/Numerics.h:111-120), JPL: I - 2 w [q]x + 2 [q]x^2"""
    qx = _skew(q[:3])
    return np.eye(3) - 2.0 * q[3] * qx + 2.0 * (qx @ qx)


def odom_pose_jacobian(q, p):
    """d(published pose error) / d(error state) of the composed state: q = qkG, p = pkG (x[0:4], x[4:7] behind the frame).  Columns: the
    reference's injected (dth, dp) (Updater.cc:549-566: R_true ~ (I - [dth x]) R); rows: the error of pGk = -R^T p and the world-frame rotation
    error phi of R_wb = R^T (R_wb,true ~ (I + [phi x]) R_wb)."""
    R = quat_to_rot(np.asarray(q, float))
    J = np.zeros((6, 6))
    J[:3, :3] = R.T @ _skew(np.asarray(p, float))
    J[:3, 3:] = -R.T
    J[3:, :3] = R.T
    return J


def odom_pose_cov(x, P):
    """NumPy mirror of rvio_odom.pose_cov (csrc/odom.hip): (C + C^T) / 2 with C = J P[0:6, 0:6] J^T, order (x, y, z, rot X, rot Y, rot Z)"""
    x, P = np.asarray(x, float), np.asarray(P, float)
    J = odom_pose_jacobian(x[0:4], x[4:7])
    Cm = J @ P[:6, :6] @ J.T
    return 0.5 * (Cm + Cm.T)


class ImuPose(C.Structure):
    """rvio_imu_pose: the pose line behind one IMU sample (rvio_hip_predict*, rvio_hip_get_imu_odometry): 104 bytes, no padding"""
    _fields_ = [("seq", C.c_int64), ("img_count", C.c_int32), ("index", C.c_int32), ("t", C.c_double),
                ("p", C.c_double * 3), ("q", C.c_double * 4), ("v", C.c_double * 3)]


IMU_POSE_DTYPE = np.dtype([("seq", "i8"), ("img_count", "i4"), ("index", "i4"), ("t", "f8"), ("p", "f8", 3), ("q", "f8", 4), ("v", "f8", 3)])
assert IMU_POSE_DTYPE.itemsize == C.sizeof(ImuPose) == 104


def _quat_norm_pos(q):
    q = q / math.sqrt(float(q @ q))
    return -q if q[3] < 0 else q


def quat_mul(a, b):
    """QuatMul (util/Numerics.h:30-63), JPL xyzw: normalised, w >= 0"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return _quat_norm_pos(np.array([aw * bx + az * by - ay * bz + ax * bw,
                                    -az * bx + aw * by + ax * bz + ay * bw,
                                    ay * bx - ax * by + aw * bz + az * bw,
                                    -ax * bx - ay * by - az * bz + aw * bw]))


def rot_to_quat(R):
    """RotToQuat (util/Numerics.h:126-167): the four-branch form, normalised, w >= 0"""
    T = R[0, 0] + R[1, 1] + R[2, 2]
    d = [R[0, 0], R[1, 1], R[2, 2]]
    q = np.zeros(4)
    big = [i for i in range(3) if d[i] > T and all(d[i] > d[j] for j in range(3) if j != i)]
    if big:
        i = big[0]
        j, k = (i + 1) % 3, (i + 2) % 3
        q[i] = math.sqrt((1 + 2 * d[i] - T) / 4)
        s = 1 / (4 * q[i])
        q[j] = s * (R[i, j] + R[j, i])
        q[k] = s * (R[i, k] + R[k, i])
        q[3] = s * (R[j, k] - R[k, j])
    else:
        q[3] = math.sqrt((1 + T) / 4)
        s = 1 / (4 * q[3])
        q[0], q[1], q[2] = s * (R[1, 2] - R[2, 1]), s * (R[2, 0] - R[0, 2]), s * (R[0, 1] - R[1, 0])
    return _quat_norm_pos(q)


def imu_preint_steps(cfg, x, imu):
    """The state half of PreIntegrator::propagate's sample loop (PreIntegrator.cc:97-179; csrc/imu_preint.h on the device) from the state head
    x[0:26], one step per sample of `imu` (abi.IMU_DTYPE).  Yields (j, u, dt, w, a, front, behind): the bias-free rate and acceleration, and
    (Rk, pk, vk, gk) in front of and behind step j.  The one statement of the recursion in this module: imu_pose_model and imu_cov_model walk it."""
    x = np.asarray(x, float)
    gR, vR, bg, ba = x[7:10].copy(), x[17:20].copy(), x[20:23], x[23:26]
    Rk, pk, vk, gk = quat_to_rot(x[10:14]), x[14:17].copy(), vR.copy(), gR.copy()
    dp, dv, Dt = np.zeros(3), np.zeros(3), 0.0
    I = np.eye(3)
    g = float(cfg.gravity)
    for j, u in enumerate(imu):
        front = (Rk, pk, vk, gk)
        dt = float(u["dt"])
        Dt += dt
        w, a = u["w"] - bg, u["a"] - ba
        w1 = math.sqrt(float(w @ w))
        wdt = w1 * dt
        wx = _skew(w)
        wx2 = wx @ wx
        if w1 < cfg.small_angle:
            dR = I - dt * wx + (dt ** 2 / 2) * wx2
            f1, f2, f3, f4 = -dt ** 3 / 3, dt ** 4 / 8, -dt ** 2 / 2, dt ** 3 / 6
        else:
            c, s = math.cos(wdt), math.sin(wdt)
            dR = I - (s / w1) * wx + ((1 - c) / w1 ** 2) * wx2
            f1 = (wdt * c - s) / w1 ** 3
            f2 = .5 * (wdt * wdt - 2 * c - 2 * wdt * s + 2) / w1 ** 4
            f3 = (c - 1) / w1 ** 2
            f4 = (wdt - s) / w1 ** 3
        Rk = dR @ Rk
        dp = dp + dv * dt
        dp = dp + Rk.T @ ((.5 * dt ** 2 * I + f1 * wx + f2 * wx2) @ a)
        dv = dv + Rk.T @ ((dt * I + f3 * wx + f4 * wx2) @ a)
        pk = vR * Dt - .5 * g * gR * Dt ** 2 + dp
        vk = Rk @ (vR - g * gR * Dt + dv)
        gk = Rk @ gR
        gk = gk / math.sqrt(float(gk @ gk))
        yield j, u, dt, w, a, front, (Rk, pk, vk, gk)


def imu_pose_model(cfg, x, imu):
    """NumPy model of csrc/imu_pose.hip: the records (abi.IMU_POSE_DTYPE; seq = 0, img_count = 0) of the IMU batch `imu` (abi.IMU_DTYPE) from
    the state head x[0:26].  imu_preint_steps on the states alone, then the pose line (System.cc:339-341) behind every sample.  Calls nothing
    from the library or the oracle: a third implementation."""
    x = np.asarray(x, float)
    qG, pG = x[0:4], x[4:7]
    RG = quat_to_rot(qG)
    out = np.zeros(len(imu), IMU_POSE_DTYPE)
    for j, u, dt, w, a, front, (Rk, pk, vk, gk) in imu_preint_steps(cfg, x, imu):
        r = out[j]
        r["index"], r["t"] = j, u["t"]
        r["p"] = RG.T @ (pk - pG)
        r["q"] = quat_mul(rot_to_quat(Rk), qG)
        r["v"] = vk
    return out


class ImuCov(C.Structure):
    """rvio_imu_cov: the covariance behind one IMU sample (rvio_hip_predict_cov*, rvio_hip_get_imu_odometry_cov): 376 bytes, no padding"""
    _fields_ = [("seq", C.c_int64), ("img_count", C.c_int32), ("index", C.c_int32), ("pose_cov", C.c_double * 36), ("vel_cov", C.c_double * 9)]


IMU_COV_DTYPE = np.dtype([("seq", "i8"), ("img_count", "i4"), ("index", "i4"), ("pose_cov", "f8", (6, 6)), ("vel_cov", "f8", (3, 3))])
assert IMU_COV_DTYPE.itemsize == C.sizeof(ImuCov) == 376
IMU_COV_COLS = (0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14)   # the columns of P11 the pose covariance reads


def imu_pose_cov_jacobian(qG, pG, qk, pk):
    """The 6 x 12 map J Vk[0:6][IMU_COV_COLS] from the errors (rot G, pos G, rot k, pos k) of the state in front of composition to the error of
    the published pose (x, y, z, rot X, rot Y, rot Z): Vk is composition's Jacobian (System.cc:345-355) at (Rk, pkG = Rk (pG - pk)), J the map of
    odom_pose_jacobian at the composed (qkG, pkG)."""
    qG, pG, qk, pk = (np.asarray(a, float) for a in (qG, pG, qk, pk))
    Rk = quat_to_rot(qk)
    pkG = Rk @ (pG - pk)
    V = np.zeros((6, 12))
    V[0:3, 0:3], V[0:3, 6:9] = Rk, np.eye(3)
    V[3:6, 3:6], V[3:6, 6:9], V[3:6, 9:12] = Rk, _skew(pkG), -Rk
    return odom_pose_jacobian(quat_mul(qk, qG), pkG) @ V


def imu_cov_model(cfg, x, P24, imu):
    """NumPy model of csrc/imu_cov.hip: the records (abi.IMU_COV_DTYPE; seq = 0, img_count = 0) of the IMU batch `imu` from the state head x[0:26]
    and the 24 x 24 head of P.  The covariance half of PreIntegrator::propagate's sample loop (PreIntegrator.cc:123-142) at the state
    imu_preint_steps has in front of every step, then per sample composition's Vk and the odometry record's map at the state behind it.  Calls
    nothing from the library or the oracle."""
    x = np.asarray(x, float)
    P = np.array(np.asarray(P24, float)[:24, :24])
    qG, pG = x[0:4], x[4:7]
    I = np.eye(3)
    g = float(cfg.gravity)
    Sig = np.diag(np.repeat([cfg.sigma_g ** 2, cfg.sigma_wg ** 2, cfg.sigma_a ** 2, cfg.sigma_wa ** 2], 3))
    cols = list(IMU_COV_COLS)
    out = np.zeros(len(imu), IMU_COV_DTYPE)
    for j, u, dt, w, a, (Rk, pk, vk, gk), behind in imu_preint_steps(cfg, x, imu):
        wx, vx = _skew(w), _skew(vk)
        F, G = np.zeros((24, 24)), np.zeros((24, 12))
        F[9:12, 9:12], F[9:12, 18:21] = -wx, -I
        F[12:15, 9:12], F[12:15, 15:18] = -Rk.T @ vx, Rk.T
        F[15:18, 6:9], F[15:18, 9:12], F[15:18, 15:18], F[15:18, 18:21], F[15:18, 21:24] = -g * Rk, -g * _skew(gk), -wx, -vx, -I
        G[9:12, 0:3], G[15:18, 0:3], G[15:18, 6:9], G[18:21, 3:6], G[21:24, 9:12] = -I, -vx, -I, I, I
        Phi = np.eye(24) + dt * F
        P = Phi @ P @ Phi.T + (dt * G) @ Sig @ G.T
        # the record behind sample j
        M = imu_pose_cov_jacobian(qG, pG, rot_to_quat(behind[0]), behind[1])
        Cm = M @ P[np.ix_(cols, cols)] @ M.T
        r = out[j]
        r["index"] = j
        r["pose_cov"] = 0.5 * (Cm + Cm.T)
        r["vel_cov"] = 0.5 * (P[15:18, 15:18] + P[15:18, 15:18].T)
    return out


# ---- auxiliary measurement update (rvio_hip_update_aux*, csrc/aux_update.hip)
RVIO_AUX_MAX_ROWS = 16
RVIO_AUX_RESIDUAL, RVIO_AUX_VALUE = 0, 1


class rvio_aux_meas(C.Structure):
    """one auxiliary measurement, host pointers: 40 bytes"""
    _fields_ = [("m", C.c_int32), ("mode", C.c_int32), ("gate", C.c_int32), ("reserved", C.c_int32),
                ("H", C.POINTER(C.c_double)), ("v", C.POINTER(C.c_double)), ("sigma", C.POINTER(C.c_double))]


assert C.sizeof(rvio_aux_meas) == 40


def make_aux_meas(H, v, sigma, mode=RVIO_AUX_RESIDUAL, gate=0):
    """an rvio_aux_meas over contiguous copies of the arrays (kept alive by the struct)"""
    H = np.ascontiguousarray(np.atleast_2d(np.asarray(H, float)))
    v, sigma = np.ascontiguousarray(v, float).reshape(-1), np.ascontiguousarray(sigma, float).reshape(-1)
    assert len(v) == len(sigma) == H.shape[0]
    dp = C.POINTER(C.c_double)
    ms = rvio_aux_meas(H.shape[0], int(mode), int(gate), 0, H.ctypes.data_as(dp), v.ctypes.data_as(dp), sigma.ctypes.data_as(dp))
    ms._keep = (H, v, sigma)
    return ms


def aux_xi(x):
    """xi(x): the additive state coordinates in error-state order (the column order of P), 0 in every rotation slot"""
    x = np.asarray(x, float)
    n = (len(x) - 26) // 7
    xi = np.zeros(24 + 6 * n)
    xi[3:9] = x[4:10]
    xi[12:24] = x[14:26]
    for p in range(n):
        xi[27 + 6 * p: 30 + 6 * p] = x[30 + 7 * p: 33 + 7 * p]
    return xi


def small_quat(e):
    """dq of an error angle (Updater.cc:549-563), JPL xyzw"""
    q = np.zeros(4)
    q[:3] = 0.5 * np.asarray(e, float)
    nrm = math.sqrt(float(q[:3] @ q[:3]))
    if nrm < 1:
        q[3] = math.sqrt(1 - nrm * nrm)
    else:
        k = 1 / math.sqrt(1 + nrm * nrm)
        q[:3] *= k
        q[3] = k
    return q


def inject_state(x, dx):
    """Updater.cc:546-613: small-angle quaternions on the rotation slots, g re-normalised, the rest additive"""
    x, dx = np.asarray(x, float), np.asarray(dx, float)
    n = (len(x) - 26) // 7
    xo = x.copy()
    xo[0:4] = quat_mul(small_quat(dx[0:3]), x[0:4])
    xo[4:10] = dx[3:9] + x[4:10]
    xo[7:10] = xo[7:10] / math.sqrt(float(xo[7:10] @ xo[7:10]))
    # (System::initialize leaves qk all zero until the first composition; QuatToRot reads it as I, and the identity is what dq multiplies)
    xo[10:14] = quat_mul(small_quat(dx[9:12]), x[10:14] if x[10:14].any() else np.array([0.0, 0.0, 0.0, 1.0]))
    xo[14:26] = dx[12:24] + x[14:26]
    for p in range(n):
        a, b = 26 + 7 * p, 24 + 6 * p
        xo[a: a + 4] = quat_mul(small_quat(dx[b: b + 3]), x[a: a + 4])
        xo[a + 4: a + 7] = dx[b + 3: b + 6] + x[a + 4: a + 7]
    return xo


def pose_line(x):
    """(pGk, qkG) of a state (System.cc:339-341): R(qG)^T (pk - pG), QuatMul(qk, qG)"""
    x = np.asarray(x, float)
    return quat_to_rot(x[0:4]).T @ (x[14:17] - x[4:7]), quat_mul(x[10:14], x[0:4])


def aux_update_model(x, P, H, v, sigma, mode=RVIO_AUX_RESIDUAL):
    """NumPy model of csrc/aux_update.hip, the arithmetic of Updater.cc:540-619 with a full-width H on whitened rows: returns (x', P', gamma).
    H: m x d in the error-state order of P; v: the residual (RESIDUAL) or the measured value z (VALUE: r = z - H xi(x)); R = diag(sigma^2).
    The textbook Joseph form, symmetrised; no gate (the caller compares gamma).  Calls nothing from the library or the oracle."""
    x, P = np.asarray(x, float), np.asarray(P, float)
    H = np.atleast_2d(np.asarray(H, float))
    v, sigma = np.asarray(v, float).reshape(-1), np.asarray(sigma, float).reshape(-1)
    m, d = H.shape
    assert P.shape == (d, d) and len(v) == m and len(sigma) == m and len(x) == 26 + 7 * ((d - 24) // 6)
    r = v - H @ aux_xi(x) if mode == RVIO_AUX_VALUE else v
    Hw, rw = H / sigma[:, None], r / sigma
    T = P @ Hw.T
    S = Hw @ T + np.eye(m)
    S = 0.5 * (S + S.T)
    K = np.linalg.solve(S, T.T).T
    gamma = abs(float(rw @ np.linalg.solve(S, rw)))
    IKH = np.eye(d) - K @ Hw
    Pn = IKH @ P @ IKH.T + K @ K.T
    return inject_state(x, K @ rw), 0.5 * (Pn + Pn.T), gamma


# ---- standstill detection (rvio_hip_standstill*, csrc/standstill.hip)
class rvio_standstill_config(C.Structure):
    """detector and update settings: 64 bytes, no padding"""
    _fields_ = [("sigma_a", C.c_double), ("sigma_w", C.c_double), ("imu_thr", C.c_double), ("disp_thr_px", C.c_double),
                ("sigma_v", C.c_double), ("sigma_bg", C.c_double),
                ("min_pairs", C.c_int32), ("bias_rows", C.c_int32), ("gate", C.c_int32), ("reserved", C.c_int32)]


class rvio_standstill(C.Structure):
    """the record of one instance: 40 bytes, no padding"""
    _fields_ = [("T", C.c_double), ("disparity", C.c_double), ("gamma", C.c_double),
                ("n_pairs", C.c_int32), ("flags", C.c_int32), ("m", C.c_int32), ("img_count", C.c_int32)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


assert C.sizeof(rvio_standstill_config) == 64 and C.sizeof(rvio_standstill) == 40
SS_IMU_STATIC, SS_IMG_STATIC, SS_IS_STATIC, SS_APPLIED = 1, 2, 4, 8


def standstill_config_default(cfg, **over):
    """the tuning values of C rvio_standstill_config_default (NOT measurements): the discrete-time form of the configured densities, twice the
    mean of T under them, half a pixel, 20 pairs, 5 cm/s"""
    c = rvio_standstill_config()
    c.sigma_a = cfg.sigma_a * math.sqrt(cfg.imu_rate)
    c.sigma_w = cfg.sigma_g * math.sqrt(cfg.imu_rate)
    c.imu_thr, c.disp_thr_px, c.sigma_v, c.sigma_bg = 12.0, 0.5, 0.05, c.sigma_w
    c.min_pairs, c.bias_rows, c.gate, c.reserved = 20, 0, 1, 0
    for k, v in over.items():
        setattr(c, k, v)
    return c


def standstill_model(x, imu, pairs_prev, pairs_cur, fx, fy, G, cfg):
    """NumPy float64 model of csrc/standstill.hip: (T, w_mean, disparity, n_pairs, flags without the `applied` bit).
    x: the state (bg = x[20:23], ba = x[23:26]); imu: abi.IMU_DTYPE records; pairs_prev / pairs_cur: the last two observations of every live
    point that has two, n x 2 NORMALISED coordinates (None or empty: no front end / no pairs); cfg: rvio_standstill_config"""
    x = np.asarray(x, float)
    w = np.asarray(imu["w"], float).reshape(-1, 3) - x[20:23]
    a = np.asarray(imu["a"], float).reshape(-1, 3) - x[23:26]
    m = len(w)
    abar = a.sum(axis=0) / m
    an = math.sqrt(float(abar @ abar))
    with np.errstate(all="ignore"):
        u = abar / an
        e = a - G * u
        T = float(((e * e).sum(axis=1) / cfg.sigma_a ** 2 + (w * w).sum(axis=1) / cfg.sigma_w ** 2).sum() / m)
    w_mean = w.sum(axis=0) / m + x[20:23]
    imu_static = an > 0 and T < cfg.imu_thr
    n_pairs, disparity = 0, 0.0
    if pairs_prev is not None and len(pairs_prev):
        d = np.asarray(pairs_cur, float).reshape(-1, 2) - np.asarray(pairs_prev, float).reshape(-1, 2)
        n_pairs = len(d)
        disparity = float(np.sqrt((fx * d[:, 0]) ** 2 + (fy * d[:, 1]) ** 2).sum() / n_pairs)
    img_static = (not cfg.disp_thr_px > 0) or n_pairs < cfg.min_pairs or disparity < cfg.disp_thr_px
    flags = (SS_IMU_STATIC if imu_static else 0) | (SS_IMG_STATIC if img_static else 0) | (SS_IS_STATIC if imu_static and img_static else 0)
    return T, w_mean, disparity, n_pairs, flags


def standstill_measurement(d, w_mean, cfg):
    """(H, z, sigma) of the standstill update for aux_update_model / rvio_hip_update_aux in VALUE mode: zero velocity at columns 15..17 and, with
    cfg.bias_rows, the mean raw gyro reading as a measurement of bg at columns 18..20"""
    rows = 6 if cfg.bias_rows else 3
    H = np.zeros((rows, d))
    for r in range(rows):
        H[r, 15 + r] = 1.0
    z = np.zeros(rows)
    sigma = np.full(rows, float(cfg.sigma_v))
    if cfg.bias_rows:
        z[3:6] = np.asarray(w_mean, float)
        sigma[3:6] = float(cfg.sigma_bg)
    return H, z, sigma


# ---- absolute fixes (rvio_hip_update_fix*, csrc/fix_rows.hip in front of the auxiliary update)
RVIO_FIX_POSITION, RVIO_FIX_ATTITUDE, RVIO_FIX_POSE, RVIO_FIX_GRAVITY = 0, 1, 2, 3
FIX_KINDS = (RVIO_FIX_POSITION, RVIO_FIX_ATTITUDE, RVIO_FIX_POSE, RVIO_FIX_GRAVITY)
FIX_ROWS = {RVIO_FIX_POSITION: 3, RVIO_FIX_ATTITUDE: 3, RVIO_FIX_POSE: 6, RVIO_FIX_GRAVITY: 3}


class rvio_fix(C.Structure):
    """one absolute fix: 128 bytes, no padding.  z[0:3]: position (POSITION, POSE) or mean raw accelerometer reading (GRAVITY); z[3:7]: quaternion
    (ATTITUDE, POSE); sigma[0:3] go with z[0:3], sigma[3:6] (rad) with the quaternion; lever: the sensed point in the IMU frame (POSITION, POSE)"""
    _fields_ = [("z", C.c_double * 7), ("sigma", C.c_double * 6), ("lever", C.c_double * 3)]


class rvio_fix_diag(C.Structure):
    """the record of one instance from the last fix: 72 bytes, no padding"""
    _fields_ = [("r", C.c_double * 6), ("gamma", C.c_double), ("applied", C.c_int32), ("kind", C.c_int32), ("m", C.c_int32), ("img_count", C.c_int32)]


FIX_DTYPE = np.dtype([("z", "f8", 7), ("sigma", "f8", 6), ("lever", "f8", 3)])
assert C.sizeof(rvio_fix) == FIX_DTYPE.itemsize == 128 and C.sizeof(rvio_fix_diag) == 72


def make_fix(p=None, q=None, sigma_p=0.0, sigma_q=0.0, lever=(0.0, 0.0, 0.0)):
    """an rvio_fix: p -> z[0:3] (position, or the accelerometer reading), q -> z[3:7]; sigma_p / sigma_q: scalars or 3-vectors"""
    f = rvio_fix()
    if p is not None:
        f.z[0:3] = [float(v) for v in p]
    if q is not None:
        f.z[3:7] = [float(v) for v in q]
    f.sigma[0:3] = [float(v) for v in np.broadcast_to(np.asarray(sigma_p, float), (3,))]
    f.sigma[3:6] = [float(v) for v in np.broadcast_to(np.asarray(sigma_q, float), (3,))]
    f.lever[0:3] = [float(v) for v in lever]
    return f


def fix_h(cfg, x, kind, lever=(0.0, 0.0, 0.0)):
    """The predicted measurement of a fix at the state x, laid out like rvio_fix.z (unused entries 0): [0:3] the world-frame position of the
    sensed point R_G^T (pk - pG + R_k^T l) (POSITION, POSE) or the accelerometer at rest ba + G R_k g (GRAVITY); [3:7] the quaternion of the
    pose line QuatMul(qk, qG) (ATTITUDE, POSE).  An all-zero qk reads as the identity."""
    x, l = np.asarray(x, float), np.asarray(lever, float)
    RG, Rk = quat_to_rot(x[0:4]), quat_to_rot(x[10:14])
    z = np.zeros(7)
    if kind in (RVIO_FIX_POSITION, RVIO_FIX_POSE):
        z[0:3] = RG.T @ (x[14:17] - x[4:7] + Rk.T @ l)
    if kind in (RVIO_FIX_ATTITUDE, RVIO_FIX_POSE):
        z[3:7] = quat_mul(x[10:14] if x[10:14].any() else np.array([0.0, 0.0, 0.0, 1.0]), x[0:4])
    if kind == RVIO_FIX_GRAVITY:
        z[0:3] = x[23:26] + cfg.gravity * (Rk @ x[7:10])
    return z


def fix_model(cfg, x, kind, fix):
    """NumPy float64 model of csrc/fix_rows.hip: (H [m x d], r [m], sigma [m]) of one fix (rvio_fix, or anything with z, sigma, lever)
    linearised at the state x, in the error-state order of P under R_true ~ (I - [dth x]) R.  The table of include/rvio_hip.h; calls nothing
    from the library or the oracle."""
    x = np.asarray(x, float)
    z, sg, l = (np.array([float(v) for v in a]) for a in (fix.z, fix.sigma, fix.lever))
    d = 24 + 6 * ((len(x) - 26) // 7)
    RG, Rk = quat_to_rot(x[0:4]), quat_to_rot(x[10:14])
    rows_H, rows_r, rows_s = [], [], []
    if kind in (RVIO_FIX_POSITION, RVIO_FIX_POSE):
        s = x[14:17] - x[4:7] + Rk.T @ l
        H = np.zeros((3, d))
        H[:, 0:3], H[:, 3:6], H[:, 9:12], H[:, 12:15] = -RG.T @ _skew(s), -RG.T, -RG.T @ Rk.T @ _skew(l), RG.T
        rows_H.append(H), rows_r.append(z[0:3] - RG.T @ s), rows_s.append(sg[0:3])
    if kind in (RVIO_FIX_ATTITUDE, RVIO_FIX_POSE):
        R = Rk @ RG
        E = quat_to_rot(z[3:7]).T @ R
        H = np.zeros((3, d))
        H[:, 0:3], H[:, 9:12] = RG.T, R.T
        rows_H.append(H), rows_r.append(0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])), rows_s.append(sg[3:6])
    if kind == RVIO_FIX_GRAVITY:
        G = float(cfg.gravity)
        gk = Rk @ x[7:10]
        H = np.zeros((3, d))
        H[:, 6:9], H[:, 9:12], H[:, 21:24] = G * Rk, G * _skew(gk), np.eye(3)
        rows_H.append(H), rows_r.append(z[0:3] - (x[23:26] + G * gk)), rows_s.append(sg[0:3])
    assert rows_H, "kind"
    return np.vstack(rows_H), np.concatenate(rows_r), np.concatenate(rows_s)


# ---- past-frame fixes (rvio_hip_update_fix_past*, csrc/fix_past.hip in front of the auxiliary update)
def _fix_past_chain(x, age):
    """(A_0 .. A_age, t_0 .. t_age): A_m rotates the IMU frame m images back into the reference frame {R}, t_m is that frame's origin in {R}.
    Clone i = n - m holds the step from the frame m back to the frame m - 1 back: A_m = A_{m-1} C_i, t_m = t_{m-1} - A_m p_i."""
    n = (len(x) - 26) // 7
    assert 0 <= age <= n, "age outside the window"
    A, t = [np.eye(3)], [np.zeros(3)]
    for m in range(1, age + 1):
        i = n - m
        A.append(A[-1] @ quat_to_rot(x[26 + 7 * i: 30 + 7 * i]))
        t.append(t[-1] - A[-1] @ x[30 + 7 * i: 33 + 7 * i])
    return A, t


def fix_past_h(x, age, lever=(0.0, 0.0, 0.0), frac=0.0):
    """The predicted measurement of a fix taken `age` images back from the state's reference frame {R} (age 0 = {R} itself, the IMU frame at
    the newest composed image; the current (qk, pk) does not enter), laid out like rvio_fix.z: [0:3] the world position of the sensed point at
    that image, R_G^T (t_a + A_a l - pG) — with frac in [0, 1) the point frac of the way towards the frame age + 1 back; [3:7] the quaternion
    world -> IMU at the frame `age` back, R = A_a^T R_G (never interpolated)."""
    x, l = np.asarray(x, float), np.broadcast_to(np.asarray(lever, float), (3,))
    frac = float(frac)
    assert 0.0 <= frac < 1.0
    RG = quat_to_rot(x[0:4])
    A, t = _fix_past_chain(x, age + (1 if frac > 0 else 0))
    z = np.zeros(7)
    z[0:3] = RG.T @ (t[age] + A[age] @ l - x[4:7])
    if frac > 0:
        z[0:3] = (1 - frac) * z[0:3] + frac * (RG.T @ (t[age + 1] + A[age + 1] @ l - x[4:7]))
    z[3:7] = rot_to_quat(A[age].T @ RG)
    return z


def _fix_past_rows(x, a, l, A, t, att):
    """the three position rows (att: attitude rows) at the whole age a"""
    n = (len(x) - 26) // 7
    RGt = quat_to_rot(x[0:4]).T
    H = np.zeros((3, 24 + 6 * n))
    if att:
        H[:, 0:3] = RGt
        for m in range(1, a + 1):
            H[:, 24 + 6 * (n - m): 27 + 6 * (n - m)] = -RGt @ A[m - 1]
        return H
    u = t[a] + A[a] @ l
    H[:, 0:3], H[:, 3:6] = -RGt @ _skew(u - x[4:7]), -RGt
    for m in range(1, a + 1):
        c = 24 + 6 * (n - m)
        H[:, c: c + 3], H[:, c + 3: c + 6] = RGt @ _skew(u - t[m - 1]) @ A[m - 1], -RGt @ A[m]
    return H


def fix_past_model(x, kind, fix, age, frac=0.0):
    """NumPy float64 model of csrc/fix_past.hip: (H [m x d], r [m], sigma [m]) of one fix (rvio_fix, or anything with z, sigma, lever) taken
    `age` images back (POSITION: frac of the way towards age + 1), linearised at the state x in the error-state order of P under
    R_true ~ (I - [dth x]) R.  The table of include/rvio_hip.h; calls nothing from the library or the oracle."""
    x, frac = np.asarray(x, float), float(frac)
    assert kind in (RVIO_FIX_POSITION, RVIO_FIX_ATTITUDE, RVIO_FIX_POSE), "kind"
    assert 0.0 <= frac < 1.0 and (frac == 0.0 or kind == RVIO_FIX_POSITION)
    z, sg, l = (np.array([float(v) for v in a]) for a in (fix.z, fix.sigma, fix.lever))
    RG = quat_to_rot(x[0:4])
    A, t = _fix_past_chain(x, age + (1 if frac > 0 else 0))
    rows_H, rows_r, rows_s = [], [], []
    if kind in (RVIO_FIX_POSITION, RVIO_FIX_POSE):
        H, h = _fix_past_rows(x, age, l, A, t, False), RG.T @ (t[age] + A[age] @ l - x[4:7])
        if frac > 0:
            H = (1 - frac) * H + frac * _fix_past_rows(x, age + 1, l, A, t, False)
            h = (1 - frac) * h + frac * (RG.T @ (t[age + 1] + A[age + 1] @ l - x[4:7]))
        rows_H.append(H), rows_r.append(z[0:3] - h), rows_s.append(sg[0:3])
    if kind in (RVIO_FIX_ATTITUDE, RVIO_FIX_POSE):
        E = quat_to_rot(z[3:7]).T @ A[age].T @ RG
        rows_H.append(_fix_past_rows(x, age, l, A, t, True))
        rows_r.append(0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])), rows_s.append(sg[3:6])
    return np.vstack(rows_H), np.concatenate(rows_r), np.concatenate(rows_s)


# ---- fixed-lag smoothed trajectory (rvio_hip_get_window*, rvio_hip_set_smoothed_odometry, csrc/window_pose.hip)
class rvio_window_pose(C.Structure):
    """the pose and covariance of the frame `age` images back from the state's reference frame: 368 bytes, no padding"""
    _fields_ = [("seq", C.c_int64), ("img_count", C.c_int32), ("age", C.c_int32), ("n_clones", C.c_int32), ("reserved", C.c_int32),
                ("p", C.c_double * 3), ("q", C.c_double * 4), ("pose_cov", C.c_double * 36)]


WINDOW_POSE_DTYPE = np.dtype([("seq", "i8"), ("img_count", "i4"), ("age", "i4"), ("n_clones", "i4"), ("reserved", "i4"),
                              ("p", "f8", 3), ("q", "f8", 4), ("pose_cov", "f8", (6, 6))])
assert WINDOW_POSE_DTYPE.itemsize == C.sizeof(rvio_window_pose) == 368


def window_pose_jacobian(x, age):
    """J (6 x d): the three POSITION rows (lever 0, frac 0) over the three ATTITUDE rows of the past-fix table at `age`"""
    x = np.asarray(x, float)
    A, t = _fix_past_chain(x, age)
    l = np.zeros(3)
    return np.vstack([_fix_past_rows(x, age, l, A, t, False), _fix_past_rows(x, age, l, A, t, True)])


def window_pose_model(x, P, age):
    """NumPy float64 model of csrc/window_pose.hip: (p, q, cov) of the frame `age` images back from the reference frame of the state x —
    p = R_G^T (t_a - pG), q = RotToQuat(A_a^T R_G) (age 0: x[0:4] as it is), cov = (C + C^T) / 2 with C = J P J^T.  Calls nothing from the
    library or the oracle."""
    x, P = np.asarray(x, float), np.asarray(P, float)
    A, t = _fix_past_chain(x, age)
    RG = quat_to_rot(x[0:4])
    p = RG.T @ (t[age] - x[4:7])
    q = x[0:4].copy() if age == 0 else rot_to_quat(A[age].T @ RG)
    J = window_pose_jacobian(x, age)
    Cm = J @ P @ J.T
    return p, q, 0.5 * (Cm + Cm.T)


def window_pose_model_as(x, P, age, dtype=np.longdouble):
    """The twin of window_pose_model evaluated in `dtype` throughout (np.longdouble: the truth the tests hold the device and the float64 model
    to): the same chain, rows and products, written out so that no intermediate passes through float64.  Returns (p, q, cov) in `dtype`."""
    x, P = np.asarray(x, dtype), np.asarray(P, dtype)
    n = (len(x) - 26) // 7
    assert 0 <= age <= n, "age outside the window"
    one, two, half = dtype(1), dtype(2), dtype(1) / dtype(2)

    def skew(w):
        S = np.zeros((3, 3), dtype)
        S[0, 1], S[0, 2], S[1, 0], S[1, 2], S[2, 0], S[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
        return S

    def q2r(q):
        qx = skew(q[:3])
        return np.eye(3, dtype=dtype) - two * q[3] * qx + two * (qx @ qx)

    def r2q(R):
        T = R[0, 0] + R[1, 1] + R[2, 2]
        d = [R[0, 0], R[1, 1], R[2, 2]]
        q = np.zeros(4, dtype)
        big = [i for i in range(3) if d[i] > T and all(d[i] > d[j] for j in range(3) if j != i)]
        if big:
            i = big[0]
            j, k = (i + 1) % 3, (i + 2) % 3
            q[i] = np.sqrt((one + two * d[i] - T) / dtype(4))
            s = one / (dtype(4) * q[i])
            q[j], q[k], q[3] = s * (R[i, j] + R[j, i]), s * (R[i, k] + R[k, i]), s * (R[j, k] - R[k, j])
        else:
            q[3] = np.sqrt((one + T) / dtype(4))
            s = one / (dtype(4) * q[3])
            q[0], q[1], q[2] = s * (R[1, 2] - R[2, 1]), s * (R[2, 0] - R[0, 2]), s * (R[0, 1] - R[1, 0])
        q = q / np.sqrt(q @ q)
        return -q if q[3] < 0 else q

    A, t = [np.eye(3, dtype=dtype)], [np.zeros(3, dtype)]
    for m in range(1, age + 1):
        i = n - m
        A.append(A[-1] @ q2r(x[26 + 7 * i: 30 + 7 * i]))
        t.append(t[-1] - A[-1] @ x[30 + 7 * i: 33 + 7 * i])
    RG = q2r(x[0:4])
    RGt = RG.T
    u = t[age]
    J = np.zeros((6, 24 + 6 * n), dtype)
    J[0:3, 0:3], J[0:3, 3:6], J[3:6, 0:3] = -RGt @ skew(u - x[4:7]), -RGt, RGt
    for m in range(1, age + 1):
        c = 24 + 6 * (n - m)
        J[0:3, c: c + 3], J[0:3, c + 3: c + 6] = RGt @ skew(u - t[m - 1]) @ A[m - 1], -RGt @ A[m]
        J[3:6, c: c + 3] = -RGt @ A[m - 1]
    Cm = J @ P @ J.T
    p = RGt @ (u - x[4:7])
    q = x[0:4].copy() if age == 0 else r2q(A[age].T @ RG)
    return p, q, half * (Cm + Cm.T)


# ---- relative-pose measurements between two frames of the window (rvio_hip_update_rel*, csrc/rel_rows.hip in front of the auxiliary update)
RVIO_REL_POSITION, RVIO_REL_ATTITUDE, RVIO_REL_POSE = 16, 17, 18      # = 16 + the fix kind
REL_KINDS = (RVIO_REL_POSITION, RVIO_REL_ATTITUDE, RVIO_REL_POSE)
REL_ROWS = {RVIO_REL_POSITION: 3, RVIO_REL_ATTITUDE: 3, RVIO_REL_POSE: 6}


def _rel_chain(x, age_new, age_old):
    """(B_0 .. B_k, s_0 .. s_k), k = age_old - age_new: the local chain from the frame age_new images back.  B_j rotates the frame j images
    further back into it, s_j is that frame's origin in it.  Clone i_j = n - age_new - j holds the step: B_j = B_{j-1} C_i, s_j = s_{j-1} - B_j p_i.
    Reads the clones n - age_old .. n - age_new - 1 and nothing else of x."""
    n = (len(x) - 26) // 7
    assert 0 <= age_new < age_old <= n, "ages outside the window, or not age_new < age_old"
    B, s = [np.eye(3)], [np.zeros(3)]
    for j in range(1, age_old - age_new + 1):
        i = n - age_new - j
        B.append(B[-1] @ quat_to_rot(x[26 + 7 * i: 30 + 7 * i]))
        s.append(s[-1] - B[-1] @ x[30 + 7 * i: 33 + 7 * i])
    return B, s


def rel_h(x, age_new, age_old, lever=(0.0, 0.0, 0.0)):
    """The predicted measurement of a delta pose between the frames age_old (b) and age_new (a < b) images back from the state's reference frame,
    laid out like rvio_fix.z: [0:3] the displacement of the sensed point from instant b to instant a in frame-b axes, B_k^T (l - s_k) - l (no
    lever: the origin of frame a in frame b, the sense of a clone's p); [3:7] the quaternion rotating frame b into frame a, R = B_k (the sense of
    a clone's q)."""
    x, l = np.asarray(x, float), np.broadcast_to(np.asarray(lever, float), (3,))
    B, s = _rel_chain(x, age_new, age_old)
    z = np.zeros(7)
    z[0:3] = B[-1].T @ (l - s[-1]) - l
    z[3:7] = rot_to_quat(B[-1])
    return z


def rel_model(x, kind, meas, age_new, age_old):
    """NumPy float64 model of csrc/rel_rows.hip: (H [m x d], r [m], sigma [m]) of one relative-pose measurement (rvio_fix, or anything with z,
    sigma, lever) between the frames age_old and age_new images back, linearised at the state x in the error-state order of P under
    R_true ~ (I - [dth x]) R.  The table of include/rvio_hip.h; calls nothing from the library or the oracle."""
    x = np.asarray(x, float)
    assert kind in REL_KINDS, "kind"
    z, sg, l = (np.array([float(v) for v in a]) for a in (meas.z, meas.sigma, meas.lever))
    n = (len(x) - 26) // 7
    B, s = _rel_chain(x, age_new, age_old)
    k = age_old - age_new
    Bk = B[k]
    rows_H, rows_r, rows_s = [], [], []
    if kind in (RVIO_REL_POSITION, RVIO_REL_POSE):
        H = np.zeros((3, 24 + 6 * n))
        for j in range(1, k + 1):
            c = 24 + 6 * (n - age_new - j)
            H[:, c: c + 3], H[:, c + 3: c + 6] = -Bk.T @ _skew(l - s[j - 1]) @ B[j - 1], Bk.T @ B[j]
        rows_H.append(H), rows_r.append(z[0:3] - (Bk.T @ (l - s[k]) - l)), rows_s.append(sg[0:3])
    if kind in (RVIO_REL_ATTITUDE, RVIO_REL_POSE):
        H = np.zeros((3, 24 + 6 * n))
        for j in range(1, k + 1):
            c = 24 + 6 * (n - age_new - j)
            H[:, c: c + 3] = B[j - 1]
        E = Bk @ quat_to_rot(z[3:7]).T
        rows_H.append(H), rows_r.append(0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])), rows_s.append(sg[3:6])
    return np.vstack(rows_H), np.concatenate(rows_r), np.concatenate(rows_s)


# ---- pose-graph export: window edges and the joint covariance of the window's poses (rvio_hip_get_window_edges*, rvio_hip_set_edge_odometry,
# rvio_hip_get_window_joint*, csrc/window_edge.hip)
class rvio_window_edge(C.Structure):
    """the relative pose of the frames age_new and age_old images back with the covariance of that quantity: 376 bytes, no padding"""
    _fields_ = [("seq", C.c_int64), ("img_count_new", C.c_int32), ("img_count_old", C.c_int32), ("age_new", C.c_int32), ("age_old", C.c_int32),
                ("n_clones", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 3), ("q", C.c_double * 4), ("cov", C.c_double * 36)]


WINDOW_EDGE_DTYPE = np.dtype([("seq", "i8"), ("img_count_new", "i4"), ("img_count_old", "i4"), ("age_new", "i4"), ("age_old", "i4"),
                              ("n_clones", "i4"), ("reserved", "i4"), ("p", "f8", 3), ("q", "f8", 4), ("cov", "f8", (6, 6))])
assert WINDOW_EDGE_DTYPE.itemsize == C.sizeof(rvio_window_edge) == 376
WINDOW_EDGE_MAX_PAIRS = 528


class _RelLever0:
    """a relative-pose measurement that only carries what the rows need: lever 0"""
    z, sigma, lever = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (0.0,) * 6, (0.0, 0.0, 0.0)


def window_edge_jacobian(x, a, b):
    """H (6 x d): the six RVIO_REL_POSE rows of rel_model between the frames a < b images back, lever 0"""
    return rel_model(x, RVIO_REL_POSE, _RelLever0, a, b)[0]


def window_edge_model(x, P, a, b):
    """NumPy float64 model of window_edge_kernel: (p, q, cov) of the edge between the frames a < b images back — p, q = rel_h at lever 0,
    cov = (C + C^T) / 2 with C = H P H^T, H = window_edge_jacobian.  Calls nothing from the library or the oracle."""
    x, P = np.asarray(x, float), np.asarray(P, float)
    z = rel_h(x, a, b)
    H = window_edge_jacobian(x, a, b)
    Cm = H @ P @ H.T
    return z[0:3], z[3:7], 0.5 * (Cm + Cm.T)


def _ops_as(dtype):
    """skew, quaternion -> rotation, rotation -> quaternion evaluated in `dtype` (the helpers of window_pose_model_as)"""
    one, two = dtype(1), dtype(2)

    def skew(w):
        S = np.zeros((3, 3), dtype)
        S[0, 1], S[0, 2], S[1, 0], S[1, 2], S[2, 0], S[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
        return S

    def q2r(q):
        qx = skew(q[:3])
        return np.eye(3, dtype=dtype) - two * q[3] * qx + two * (qx @ qx)

    def r2q(R):
        T = R[0, 0] + R[1, 1] + R[2, 2]
        d = [R[0, 0], R[1, 1], R[2, 2]]
        q = np.zeros(4, dtype)
        big = [i for i in range(3) if d[i] > T and all(d[i] > d[j] for j in range(3) if j != i)]
        if big:
            i = big[0]
            j, k = (i + 1) % 3, (i + 2) % 3
            q[i] = np.sqrt((one + two * d[i] - T) / dtype(4))
            s = one / (dtype(4) * q[i])
            q[j], q[k], q[3] = s * (R[i, j] + R[j, i]), s * (R[i, k] + R[k, i]), s * (R[j, k] - R[k, j])
        else:
            q[3] = np.sqrt((one + T) / dtype(4))
            s = one / (dtype(4) * q[3])
            q[0], q[1], q[2] = s * (R[1, 2] - R[2, 1]), s * (R[2, 0] - R[0, 2]), s * (R[0, 1] - R[1, 0])
        q = q / np.sqrt(q @ q)
        return -q if q[3] < 0 else q

    return skew, q2r, r2q


def window_edge_model_as(x, P, a, b, dtype=np.longdouble):
    """The twin of window_edge_model evaluated in `dtype` throughout (np.longdouble: the truth the tests hold the device and the float64 model
    to): the same chain, rows and products, written out so that no intermediate passes through float64.  Returns (p, q, cov) in `dtype`."""
    x, P = np.asarray(x, dtype), np.asarray(P, dtype)
    n = (len(x) - 26) // 7
    assert 0 <= a < b <= n, "ages outside the window, or not a < b"
    skew, q2r, r2q = _ops_as(dtype)
    k = b - a
    B, s = [np.eye(3, dtype=dtype)], [np.zeros(3, dtype)]
    for j in range(1, k + 1):
        i = n - a - j
        B.append(B[-1] @ q2r(x[26 + 7 * i: 30 + 7 * i]))
        s.append(s[-1] - B[-1] @ x[30 + 7 * i: 33 + 7 * i])
    Bkt = B[k].T
    H = np.zeros((6, 24 + 6 * n), dtype)
    for j in range(1, k + 1):
        c = 24 + 6 * (n - a - j)
        H[0:3, c: c + 3], H[0:3, c + 3: c + 6] = Bkt @ skew(s[j - 1]) @ B[j - 1], Bkt @ B[j]
        H[3:6, c: c + 3] = B[j - 1]
    Cm = H @ P @ H.T
    return -(Bkt @ s[k]), r2q(B[k]), (dtype(1) / dtype(2)) * (Cm + Cm.T)


def window_joint_model(x, P, m):
    """NumPy float64 model of window_joint_kernel: the joint covariance (6 m x 6 m) of the world poses of the ages 0 .. m - 1, newest first —
    block (a, b) = J_a P J_b^T with J = window_pose_jacobian, the diagonal blocks symmetrised like window_pose_model's — exactly symmetric.
    Calls nothing from the library or the oracle."""
    x, P = np.asarray(x, float), np.asarray(P, float)
    J = [window_pose_jacobian(x, a) for a in range(m)]
    X = np.zeros((6 * m, 6 * m))
    for a in range(m):
        T = P @ J[a].T
        Cm = J[a] @ P @ J[a].T              # (window_pose_model's order of products: the same bits)
        X[6 * a: 6 * a + 6, 6 * a: 6 * a + 6] = 0.5 * (Cm + Cm.T)
        for b in range(a):
            Xba = J[b] @ T
            X[6 * b: 6 * b + 6, 6 * a: 6 * a + 6], X[6 * a: 6 * a + 6, 6 * b: 6 * b + 6] = Xba, Xba.T
    return X


def window_pose_jacobian_as(x, age, dtype=np.longdouble):
    """window_pose_jacobian evaluated in `dtype` throughout (the J of window_pose_model_as)"""
    x = np.asarray(x, dtype)
    n = (len(x) - 26) // 7
    assert 0 <= age <= n, "age outside the window"
    skew, q2r, _ = _ops_as(dtype)
    A, t = [np.eye(3, dtype=dtype)], [np.zeros(3, dtype)]
    for m in range(1, age + 1):
        i = n - m
        A.append(A[-1] @ q2r(x[26 + 7 * i: 30 + 7 * i]))
        t.append(t[-1] - A[-1] @ x[30 + 7 * i: 33 + 7 * i])
    RGt = q2r(x[0:4]).T
    u = t[age]
    J = np.zeros((6, 24 + 6 * n), dtype)
    J[0:3, 0:3], J[0:3, 3:6], J[3:6, 0:3] = -RGt @ skew(u - x[4:7]), -RGt, RGt
    for m in range(1, age + 1):
        c = 24 + 6 * (n - m)
        J[0:3, c: c + 3], J[0:3, c + 3: c + 6] = RGt @ skew(u - t[m - 1]) @ A[m - 1], -RGt @ A[m]
        J[3:6, c: c + 3] = -RGt @ A[m - 1]
    return J


def window_joint_model_as(x, P, m, dtype=np.longdouble):
    """The twin of window_joint_model evaluated in `dtype` throughout: every block J_a P J_b^T, the whole matrix symmetrised"""
    P = np.asarray(P, dtype)
    J = np.vstack([window_pose_jacobian_as(x, a, dtype) for a in range(m)])
    X = J @ P @ J.T
    return (dtype(1) / dtype(2)) * (X + X.T)


def window_edge_from_poses(x, a, b, dtype=float):
    """G (6 x 12): the first-order map from the world-pose errors of the frames a and b (each in pose_cov's convention: the position error, then
    the world-frame rotation error phi, frame a's six first) to the error of the edge (a, b) in rvio_window_edge.cov's convention, so that
    G Joint[{a, b}] G^T = the edge's cov exactly (the chain rule: H = G [J_a; J_b]).  With W_f = R(q_f)^T (IMU at frame f -> world) and
    p_f the world positions: dp = W_b^T (dp_a - dp_b) + W_b^T [(p_a - p_b) x] phi_b, dth = W_a^T (phi_a - phi_b)."""
    x = np.asarray(x, dtype)
    n = (len(x) - 26) // 7
    skew, q2r, _ = _ops_as(np.dtype(dtype).type)
    dt = np.dtype(dtype).type

    def pose(age):
        A, t = np.eye(3, dtype=dt), np.zeros(3, dt)
        for m in range(1, age + 1):
            i = n - m
            A = A @ q2r(x[26 + 7 * i: 30 + 7 * i])
            t = t - A @ x[30 + 7 * i: 33 + 7 * i]
        RG = q2r(x[0:4])
        return RG.T @ (t - x[4:7]), RG.T @ A          # p_f, W_f

    pa, Wa = pose(a)
    pb, Wb = pose(b)
    G = np.zeros((6, 12), dt)
    G[0:3, 0:3], G[0:3, 6:9], G[0:3, 9:12] = Wb.T, -Wb.T, Wb.T @ skew(pa - pb)
    G[3:6, 3:6], G[3:6, 9:12] = Wa.T, -Wa.T
    return G


# ---- landmark covariance: the 3 x 3 uncertainty of every cloud point (rvio_hip_set_landmark_cov, rvio_hip_get_landmark_cov*, csrc/landmark_cov.hip)
class rvio_landmark_cov(C.Structure):
    """one cloud point with its covariance in {R} and in the world frame of the PRIOR state: 224 bytes, no padding"""
    _fields_ = [("feat", C.c_int32), ("n_obs", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32), ("rho", C.c_double),
                ("rho_sigma", C.c_double), ("p_r", C.c_double * 3), ("p_w", C.c_double * 3), ("cov_r", C.c_double * 9), ("cov_w", C.c_double * 9)]


LANDMARK_COV_DTYPE = np.dtype([("feat", "i4"), ("n_obs", "i4"), ("status", "i4"), ("reserved", "i4"), ("rho", "f8"), ("rho_sigma", "f8"),
                               ("p_r", "f8", 3), ("p_w", "f8", 3), ("cov_r", "f8", (3, 3)), ("cov_w", "f8", (3, 3))])
assert LANDMARK_COV_DTYPE.itemsize == C.sizeof(rvio_landmark_cov) == 224
LANDMARK_COV_OK, LANDMARK_COV_SINGULAR = 0, 1
LANDMARK_COV_PIVOT_EPS = 64 * 2.0 ** -52      # LP_LMC_PIVOT_EPS of csrc/launch_plan.h: a Cholesky pivot of N at or below this share of its diagonal entry is not positive


def landmark_sigma(cfg):
    """the normalised pixel sigma of the update (Updater.cc:42-44): max(sigma_px, sigma_py) as a float widened to double"""
    return float(max(np.float32(cfg.sigma_px), np.float32(cfg.sigma_py)))


def _feature_rows_as(cal, x, ftype, L, pf, dt, with_hx=True, first_exact=False):
    """The measurement model of one feature at the triple pf = (phi, psi, rho), every operation in the scalar type `dt`: the relative-pose chain
    over the nPh = L - 1 clones of the track and the raw rows of all L observations.  Shared by landmark_cov_model_as and
    feature_update_model_as.  Written in the point scaled by rho, Y_i = rho X_i (Y_0 = R_ic e + rho t_ic, Y_{i+1} = R_i (Y_i - rho p_i)), so
    that rho = 0 (no parallax) is an ordinary argument:
      h_i = R_ci (Y_i - rho t_ic)  (the predicted pixel is h_i[:2] / h_i[2]),   Hf_i = Hp_i [R_ci RI_i R_ic Jang | R_ci ((RI_i - I) t_ic + tI_i)],
      Hx_i[clone j < i] = Hp_i R_ci RI_i RI_{j+1}^T [ [Y_{j+1} x] | -rho R_j ]
    first_exact: the first observation as Updater.cc:186-206,297-313 take it — h_0 = e and Hf_0 = Hp_0 Jang, without the factor R_ci R_ic, which is
    the identity only as far as the configured extrinsic rotation is orthonormal (the EuRoC T_bc: to 6e-13).
    Returns a dict: x (as dt), n, nPh, c0 (the first clone of the track), rho, e, Jang, Ric, tic, R, RI, tI, Y (lists over the chain), h (L x 3), Hf
    (2L x 3), Hx (2L x 6n; zeros when with_hx is False)."""
    x = np.asarray(x, dt)
    n = (len(x) - 26) // 7
    L = int(L)
    nPh = L - 1
    one = "1" if ftype in ("1", b"1", ord("1")) else "2"
    assert ftype in ("1", b"1", ord("1"), "2", b"2", ord("2")) and 1 <= nPh <= n
    skew, q2r, _ = _ops_as(dt)
    T = np.array([dt(v) for v in cal.T_bc]).reshape(4, 4)
    Ric, tic = T[0:3, 0:3], T[0:3, 3]
    Rci = Ric.T
    c0 = n - nPh if one == "1" else 0
    phi, psi, rho = (dt(v) for v in pf)
    e = np.array([np.cos(phi) * np.sin(psi), np.sin(phi), np.cos(phi) * np.cos(psi)], dt)
    Jang = np.array([[-np.sin(phi) * np.sin(psi), np.cos(phi) * np.cos(psi)], [np.cos(phi), dt(0)],
                     [-np.sin(phi) * np.cos(psi), -np.cos(phi) * np.sin(psi)]], dt)
    I3 = np.eye(3, dtype=dt)
    R, Y, RI, tI = [], [Ric @ e + rho * tic], [I3], [np.zeros(3, dt)]
    for i in range(nPh):
        a = 26 + 7 * (c0 + i)
        Ri = q2r(x[a: a + 4])
        R.append(Ri)
        Y.append(Ri @ (Y[-1] - rho * x[a + 4: a + 7]))
        tI.append(Ri @ (tI[-1] - x[a + 4: a + 7]))
        RI.append(Ri @ RI[-1])
    h, Hf, Hx = np.zeros((L, 3), dt), np.zeros((2 * L, 3), dt), np.zeros((2 * L, 6 * n), dt)
    for i in range(L):
        exact0 = first_exact and i == 0
        h[i] = e if exact0 else Rci @ (Y[i] - rho * tic)               # rho times the point in camera i (t_ci = -R_ci t_ic)
        Hp = np.array([[1 / h[i, 2], dt(0), -h[i, 0] / (h[i, 2] * h[i, 2])], [dt(0), 1 / h[i, 2], -h[i, 1] / (h[i, 2] * h[i, 2])]], dt)
        tc = Rci @ ((RI[i] - I3) @ tic + tI[i])
        Hf[2 * i: 2 * i + 2, 0:2] = Hp @ Jang if exact0 else Hp @ (Rci @ RI[i] @ Ric @ Jang)
        Hf[2 * i: 2 * i + 2, 2] = Hp @ tc
        for j in range(i if with_hx else 0):
            c = 6 * (c0 + j)
            Hx[2 * i: 2 * i + 2, c: c + 6] = Hp @ Rci @ ((RI[i] @ RI[j + 1].T) @ np.hstack([skew(Y[j + 1]), -rho * R[j]]))
    return dict(x=x, n=n, nPh=nPh, c0=c0, rho=rho, e=e, Jang=Jang, Ric=Ric, tic=tic, R=R, RI=RI, tI=tI, Y=Y, h=h, Hf=Hf, Hx=Hx)


def landmark_cov_model_as(cal, x, P, ftype, L, meas, pf, dtype=np.longdouble, sigma=None, hf_only=False):
    """The covariance of one cloud point evaluated in `dtype` throughout (np.longdouble: the truth the tests hold the device and the float64
    model to).  cal: anything with T_bc (rvio_config, rvio_calibration); x, P: the state and covariance the update READ; ftype: '1' / '2' (or
    their codes); L: the track length, all L observations enter (the halving of Updater.cc:271-275 concerns the update, not the triangulation);
    pf = (phi, psi, rho): the stored inverse-depth estimate in the first camera frame; meas is accepted for symmetry with oracle.feature_model
    and not read: the Jacobians are evaluated at pf.  sigma: the normalised pixel sigma (None: landmark_sigma(cal), which needs an rvio_config).

    With the chain X_0 = R_ic e / rho + t_ic, X_{i+1} = R_i (X_i - p_i) over the nPh = L - 1 clones of the track (the IMU-frame point at every
    image of the track) and RI_i = R_{i-1} .. R_0:
      Hf_i = Hp_i [R_ci RI_i R_ic Jang | R_ci ((RI_i - I) t_ic + tI_i)],   Hx_i[clone j < i] = rho Hp_i R_ci RI_i RI_{j+1}^T [ [X_{j+1} x] | -R_j ]
      N = Hf^T Hf,  A = N^-1 Hf^T,  Jth = RI_nPh R_ic [Jang / rho | -e / rho^2],  Jx[clone j] = RI_nPh RI_{j+1}^T [ [X_{j+1} x] | -R_j ]
      M = Jx - Jth A Hx,   cov_r = sigma^2 Jth N^-1 Jth^T + M P_span M^T
      p_w = R_G^T (p_r - pG),   M_w = R_G^T [ -[(p_r - pG) x] | -I | M ],   cov_w = sigma^2 (R_G^T Jth) N^-1 (R_G^T Jth)^T + M_w P M_w^T
      rho_sigma^2 = (sigma^2 N^-1 + (A Hx) P_span (A Hx)^T)_22
    in the error convention of P (inject_state: R_true ~ (I - [dth x]) R, positions additive).  Returns a dict; status 1 (a Cholesky pivot of N
    at or below LANDMARK_COV_PIVOT_EPS of its diagonal entry): the covariances and rho_sigma are NaN, the points are filled.  hf_only: stop
    behind Hf and the points (P is not read; what a Gauss-Newton triangulation needs per step).  Calls nothing from the library or the oracle."""
    dt = np.dtype(dtype).type
    P = None if hf_only else np.asarray(P, dt)
    c = _feature_rows_as(cal, x, ftype, L, pf, dt, with_hx=not hf_only)
    x, n, nPh, c0, rho, e, Jang, Ric, R, RI, Hf, Hx = (c[k] for k in ("x", "n", "nPh", "c0", "rho", "e", "Jang", "Ric", "R", "RI", "Hf", "Hx"))
    d = 24 + 6 * n
    L = int(L)
    skew, q2r, _ = _ops_as(dt)
    sig = dt(landmark_sigma(cal) if sigma is None else sigma)
    X = [Y / rho for Y in c["Y"]]                       # the IMU-frame point at every image of the track

    def D(i, j):   # d X_i / d (error of clone j), j < i
        return (RI[i] @ RI[j + 1].T) @ np.hstack([skew(X[j + 1]), -R[j]])

    if hf_only:
        RG = q2r(x[0:4])
        return dict(Hf=Hf, p_r=X[nPh], p_w=RG.T @ (X[nPh] - x[4:7]))
    N = Hf.T @ Hf
    # 3 x 3 Cholesky, the pivots held to their diagonal entries
    Lc, status = np.zeros((3, 3), dt), LANDMARK_COV_OK
    for k in range(3):
        piv = N[k, k] - Lc[k, :k] @ Lc[k, :k]
        if not piv > dt(LANDMARK_COV_PIVOT_EPS) * N[k, k]:
            status = LANDMARK_COV_SINGULAR
            break
        Lc[k, k] = np.sqrt(piv)
        for i in range(k + 1, 3):
            Lc[i, k] = (N[i, k] - Lc[i, :k] @ Lc[k, :k]) / Lc[k, k]
    Jth = RI[nPh] @ Ric @ np.hstack([Jang / rho, (-e / (rho * rho)).reshape(3, 1)])
    Jx = np.zeros((3, 6 * n), dt)
    for j in range(nPh):
        Jx[:, 6 * (c0 + j): 6 * (c0 + j) + 6] = D(nPh, j)
    RG = q2r(x[0:4])
    p_r = X[nPh]
    p_w = RG.T @ (p_r - x[4:7])
    out = dict(status=status, n_obs=int(L), rho=rho, p_r=p_r, p_w=p_w, Hf=Hf, Hx=Hx, N=N, Jtheta=Jth, Jx=Jx, span=(24 + 6 * c0, 24 + 6 * (c0 + nPh)))
    nan3 = np.full((3, 3), np.nan, dt)
    if status != LANDMARK_COV_OK:
        out.update(cov_r=nan3, cov_w=nan3.copy(), rho_sigma=dt(np.nan), cov_theta=nan3.copy(), M=None, M_w=None)
        return out
    Li = np.zeros((3, 3), dt)                          # L^-1 by forward substitution, N^-1 = L^-T L^-1
    for c in range(3):
        for r in range(c, 3):
            Li[r, c] = ((dt(1) if r == c else dt(0)) - Lc[r, c:r] @ Li[c:r, c]) / Lc[r, r]
    Ninv = Li.T @ Li
    AHx = Ninv @ (Hf.T @ Hx)
    M = np.zeros((3, d), dt)
    M[:, 24:] = Jx - Jth @ AHx
    Mw = RG.T @ M
    Mw[:, 0:3], Mw[:, 3:6] = -RG.T @ skew(p_r - x[4:7]), -RG.T
    half = dt(1) / dt(2)
    Cr = sig * sig * (Jth @ Ninv @ Jth.T) + M @ P @ M.T
    Jw = RG.T @ Jth
    Cw = sig * sig * (Jw @ Ninv @ Jw.T) + Mw @ P @ Mw.T
    Ct = sig * sig * Ninv + AHx @ P[24:, 24:] @ AHx.T
    out.update(cov_r=half * (Cr + Cr.T), cov_w=half * (Cw + Cw.T), cov_theta=half * (Ct + Ct.T), rho_sigma=np.sqrt(Ct[2, 2]), M=M, M_w=Mw, A=Ninv @ Hf.T)
    return out


def landmark_cov_model(cal, x, P, ftype, L, meas, pf, sigma=None, hf_only=False):
    """NumPy float64 model of csrc/landmark_cov.hip with analytic Jacobians: landmark_cov_model_as evaluated in float64 (see there)"""
    return landmark_cov_model_as(cal, x, P, ftype, L, meas, pf, dtype=np.float64, sigma=sigma, hf_only=hf_only)


# ---- the per-feature stage of the update (U3 .. U5 of Updater::update and the feature's share of the information block) at a GIVEN triple
def _nullspace_rows_as(Hf, Hx, r, N, dt, basis):
    """(Hn, rn): the rows of Q2^T [Hx | r], Q2 an orthonormal basis of the left nullspace of the first N columns of Hf, every operation in dt.
    basis 'householder': N reflectors; 'givens': the reference's sweep (Updater.cc:370-402: column by column, rows bottom-up, each rotation
    built from the pair it zeroes).  Both leave the rows N .. M - 1; what is formed from them (gamma, A, b) does not depend on the choice."""
    M = Hf.shape[0]
    W = np.hstack([Hf[:, :N], Hx, r.reshape(M, 1)]).astype(dt)
    if basis == "householder":
        for k in range(N):
            v = W[k:, k].copy()
            nv = np.sqrt(v @ v)
            if nv == 0:
                continue
            v[0] += nv if v[0] >= 0 else -nv
            W[k:, :] -= np.outer(v, (dt(2) / (v @ v)) * (v @ W[k:, :]))
    else:
        assert basis == "givens"
        for k in range(N):
            for m in range(M - 1, k, -1):
                p, q = W[m - 1, k], W[m, k]
                nn = np.sqrt(p * p + q * q)
                if nn == 0:
                    continue
                c, s = p / nn, q / nn
                a, b = W[m - 1, :].copy(), W[m, :].copy()
                W[m - 1, :], W[m, :] = c * a + s * b, c * b - s * a
    return W[N:, N: N + Hx.shape[1]], W[N:, -1]


def feature_update_model_as(cal, x, P, ftype, L, meas, pf, dtype=np.longdouble, sigma=None, basis="householder"):
    """What the per-feature stage of the update hands on for ONE feature, evaluated in `dtype` throughout at the given triple pf = (phi, psi,
    rho) — np.longdouble: the truth the tests hold the device's gate and information share to.  All L observations went into pf; the rows are
    the first Lu = L (type '1') or ceil(L / 2) (type '2', Updater.cc:271-275) of them, the columns start at clone n - (Lu - 1) (type '1') or 0.
      r      measurement minus predicted pixel; the pixel is rounded to float32 and the difference taken in float32 (Updater.cc:307-308,338-339)
      N      2 if |Hf[:, 2]| < 1e-4 (no depth column to project out, Updater.cc:372-377), else 3;  ndof = 2 Lu - N
      Q_f    an orthonormal basis of the span of the first N columns of Hf;  Hn = Q2^T Hx, rn = Q2^T r over its complement
      gamma  rn^T (Hn Pcc Hn^T + sigma^2 I)^-1 rn  by a Cholesky factorisation written out in dtype (np.linalg would drop to float64)
      A, b   Hx^T (I - Q_f Q_f^T) Hx  (6n x 6n) and Hx^T (I - Q_f Q_f^T) r  (6n): the feature's share of the information block
    None of these depends on the basis chosen (`basis`: 'householder' or the reference's 'givens' sweep).  Returns dict(N, ndof, gamma, A, b,
    S_cond = cond(Hn Pcc Hn^T + sigma^2 I) (a float64 figure), Lu, cols = (cLo, cHi) the feature's non-zero column range, r, rn_norm, hf2 =
    |Hf[:, 2]|, r_norm = |r| and hx_norms = the column norms of Hx before the projection: the scales of a backward error).  The chain and the
    raw rows are _feature_rows_as, shared with landmark_cov_model_as; nothing from the library or the oracle."""
    dt = np.dtype(dtype).type
    c = _feature_rows_as(cal, x, ftype, L, pf, dt, first_exact=True)
    n = c["n"]
    one = "1" if ftype in ("1", b"1", ord("1")) else "2"
    Lu = int(L) if one == "1" else (int(L) + 1) // 2
    M = 2 * Lu
    Hf, Hx = c["Hf"][:M], c["Hx"][:M]
    z = np.asarray(meas, np.float32)[:Lu]
    px = np.stack([c["h"][:Lu, 0] / c["h"][:Lu, 2], c["h"][:Lu, 1] / c["h"][:Lu, 2]], axis=1).astype(np.float32)
    r32 = (z - px).astype(np.float32).reshape(-1)
    r = r32.astype(dt)
    hf2 = np.sqrt(Hf[:, 2] @ Hf[:, 2])
    N = 2 if hf2 < dt(1e-4) else 3
    Hn, rn = _nullspace_rows_as(Hf, Hx, r, N, dt, basis)
    ndof = M - N
    sig = dt(landmark_sigma(cal) if sigma is None else sigma)
    Pcc = np.asarray(P, dt)[24:, 24:]
    S = Hn @ Pcc @ Hn.T
    S = (dt(1) / dt(2)) * (S + S.T) + sig * sig * np.eye(ndof, dtype=dt)
    Lc = np.zeros((ndof, ndof), dt)
    for k in range(ndof):
        Lc[k, k] = np.sqrt(S[k, k] - Lc[k, :k] @ Lc[k, :k])
        for i in range(k + 1, ndof):
            Lc[i, k] = (S[i, k] - Lc[i, :k] @ Lc[k, :k]) / Lc[k, k]
    y = np.zeros(ndof, dt)
    for k in range(ndof):
        y[k] = (rn[k] - Lc[k, :k] @ y[:k]) / Lc[k, k]
    c0 = n - (Lu - 1) if one == "1" else 0
    return dict(N=N, ndof=ndof, gamma=y @ y, A=Hn.T @ Hn, b=Hn.T @ rn, S_cond=float(np.linalg.cond(S.astype(np.float64))), Lu=Lu,
                cols=(6 * c0, 6 * (c0 + Lu - 1)), r=r32, rn_norm=np.sqrt(rn @ rn), hf2=hf2, r_norm=np.sqrt(r @ r), hx_norms=np.sqrt(np.sum(Hx * Hx, axis=0)))


def feature_update_model(cal, x, P, ftype, L, meas, pf, sigma=None, basis="householder"):
    """NumPy float64 model of the per-feature stage at a given triple: feature_update_model_as evaluated in float64 (see there)"""
    return feature_update_model_as(cal, x, P, ftype, L, meas, pf, dtype=np.float64, sigma=sigma, basis=basis)


# ---- map landmarks: pixel observations of known world points (rvio_hip_update_map*, csrc/map_rows.hip in front of the auxiliary update)
RVIO_MAP_NORMALISED, RVIO_MAP_PIXELS = 0, 1
RVIO_MAP_MAX_POINTS = 8
MAP_USED, MAP_GATED, MAP_REJECTED, MAP_EMPTY = 0, 1, 2, 3
MAP_MIN_DEPTH = 0.1            # LP_MAP_MIN_DEPTH of csrc/launch_plan.h: a tuning value, not a measurement
MAP_CHI2_95_2 = 5.991465       # chi2inv(0.95, 2) as csrc/chi2_table.inc holds it (6 decimals): the per-point gate


class rvio_map_obs(C.Structure):
    """one observation of a known world point: 48 bytes, no padding.  p_w: the point in the filter's world frame; uv: normalised coordinates or
    raw pixels (units); sigma: of uv, in its units"""
    _fields_ = [("p_w", C.c_double * 3), ("uv", C.c_double * 2), ("sigma", C.c_double)]


class rvio_map_point(C.Structure):
    """what became of one slot: 40 bytes, no padding.  status: 0 used, 1 gated out, 2 rejected, 3 empty slot"""
    _fields_ = [("r", C.c_double * 2), ("gamma", C.c_double), ("depth", C.c_double), ("status", C.c_int32), ("reserved", C.c_int32)]


class rvio_map_diag(C.Structure):
    """the record of one instance from the last map call: 32 bytes, no padding"""
    _fields_ = [("gamma", C.c_double), ("applied", C.c_int32), ("m", C.c_int32), ("n_used", C.c_int32), ("n_obs", C.c_int32),
                ("img_count", C.c_int32), ("reserved", C.c_int32)]


MAP_OBS_DTYPE = np.dtype([("p_w", "f8", 3), ("uv", "f8", 2), ("sigma", "f8")])
assert C.sizeof(rvio_map_obs) == MAP_OBS_DTYPE.itemsize == 48 and C.sizeof(rvio_map_point) == 40 and C.sizeof(rvio_map_diag) == 32


def make_map_obs(points):
    """a ctypes array of rvio_map_obs from (p_w, uv, sigma) triples"""
    arr = (rvio_map_obs * len(points))()
    for o, (p_w, uv, sigma) in zip(arr, points):
        o.p_w[0:3] = [float(v) for v in p_w]
        o.uv[0:2] = [float(v) for v in uv]
        o.sigma = float(sigma)
    return arr


def _map_cam(cal):
    """(Rci, tci) of anything with T_bc (rvio_config, rvio_calibration), as csrc/rvio_hip.hip fill_camcal forms them"""
    T = np.array([float(v) for v in cal.T_bc]).reshape(4, 4)
    Rci = T[0:3, 0:3].T.copy()
    return Rci, -(Rci @ T[0:3, 3])


def map_h(cal, x, age, p_w):
    """(H [2 x d], h [2], depth) of one known world point p_w seen by the camera of calibration `cal` at the image `age` back from the state's
    reference frame {R}: h the predicted normalised image coordinates, H its Jacobian in the error-state order of P under
    R_true ~ (I - [dth x]) R.  The table of include/rvio_hip.h; calls nothing from the library or the oracle."""
    x, f = np.asarray(x, float), np.asarray(p_w, float)
    n = (len(x) - 26) // 7
    Rci, tci = _map_cam(cal)
    A, t = _fix_past_chain(x, age)
    RGf = quat_to_rot(x[0:4]) @ f
    w = RGf + x[4:7]
    pC = Rci @ (A[age].T @ (w - t[age])) + tci
    depth = float(pC[2])
    with np.errstate(all="ignore"):
        h = np.array([pC[0] / depth, pC[1] / depth])
        M = (np.array([[1.0, 0.0, -h[0]], [0.0, 1.0, -h[1]]]) / depth) @ Rci @ A[age].T
    H = np.zeros((2, 24 + 6 * n))
    H[:, 0:3], H[:, 3:6] = M @ _skew(RGf), M
    for m in range(1, age + 1):
        c = 24 + 6 * (n - m)
        H[:, c: c + 3], H[:, c + 3: c + 6] = -M @ _skew(w - t[m - 1]) @ A[m - 1], M @ A[m]
    return H, h, depth


def map_model(cal, x, P, obs, age, units, gate_each, uv_n=None, hold=None):
    """NumPy float64 model of csrc/map_rows.hip: (H [2 n x d], r [2 n], sigma [2 n], gamma [n], status [n]) of n = len(obs) <= 8 observations
    (rvio_map_obs, or anything with p_w, uv, sigma) at the image `age` back.  PIXELS: uv_n holds the undistorted normalised coordinates of the
    float pixels (n x 2, the tracker's undistortion: the model has none of its own) and the rows get sigma / |fx|, sigma / |fy|.  A slot that is
    rejected (depth < MAP_MIN_DEPTH or a non-finite projection) or, with gate_each, gated out (|gamma_j| >= chi2inv(0.95, 2) against P as it
    is, or a non-positive pivot) has H = 0, r = 0, sigma = 1 in its two rows.
    hold: (gamma of pass 0, status of the pass before) of an iterated update — a later pass: a slot that is not used keeps its status, a used
    one keeps its gamma and is not gated again (it may still be rejected at the new state, and then stays so)."""
    x, P = np.asarray(x, float), np.asarray(P, float)
    assert units in (RVIO_MAP_NORMALISED, RVIO_MAP_PIXELS) and 1 <= len(obs) <= RVIO_MAP_MAX_POINTS
    assert units == RVIO_MAP_NORMALISED or uv_n is not None, "PIXELS: pass the undistorted coordinates"
    d = P.shape[0]
    nob = len(obs)
    H, r, sg = np.zeros((2 * nob, d)), np.zeros(2 * nob), np.ones(2 * nob)
    gamma, status = np.zeros(nob), np.zeros(nob, int)
    for j, o in enumerate(obs):
        if hold is not None and hold[1][j] != MAP_USED:
            gamma[j], status[j] = hold[0][j], hold[1][j]
            continue
        Hj, h, depth = map_h(cal, x, age, [float(v) for v in o.p_w])
        z = np.array([float(v) for v in o.uv]) if units == RVIO_MAP_NORMALISED else np.asarray(uv_n, float).reshape(-1, 2)[j]
        s = float(o.sigma)
        sj = np.array([s, s]) if units == RVIO_MAP_NORMALISED else np.array([s / abs(float(cal.fx)), s / abs(float(cal.fy))])
        rj = z - h
        if not (np.isfinite(depth) and depth >= MAP_MIN_DEPTH and np.all(np.isfinite(h)) and np.all(np.isfinite(rj)) and np.all(sj > 0) and np.all(np.isfinite(sj))):
            status[j] = MAP_REJECTED
            continue
        if hold is not None:
            gamma[j] = hold[0][j]
            H[2 * j: 2 * j + 2], r[2 * j: 2 * j + 2], sg[2 * j: 2 * j + 2] = Hj, rj, sj
            continue
        Hw, rw = Hj / sj[:, None], rj / sj
        S = Hw @ P @ Hw.T + np.eye(2)
        d0 = S[0, 0]
        l = S[0, 1] / d0 if d0 > 0 else 0.0
        d1 = S[1, 1] - l * S[0, 1]
        if not (d0 > 0 and d1 > 0):
            status[j] = MAP_GATED
            continue
        gamma[j] = abs(rw[0] * rw[0] / d0 + (rw[1] - l * rw[0]) ** 2 / d1)
        if gate_each and not gamma[j] < MAP_CHI2_95_2:
            status[j] = MAP_GATED
            continue
        H[2 * j: 2 * j + 2], r[2 * j: 2 * j + 2], sg[2 * j: 2 * j + 2] = Hj, rj, sj
    return H, r, sg, gamma, status


# ---- iterated measurement updates (rvio_hip_set_meas_iterations: the fix, past-fix, rel and map families relinearised on the device)
RVIO_MEAS_MAX_ITERS = 8


class rvio_meas_iter(C.Structure):
    """what the iterated update made of one instance in the last fix / past-fix / rel / map call: 24 bytes, no padding.  iterations: passes run;
    step: max |dx_new - dx| of the last one; converged: step < tol; gamma0: pass 0's gamma (the innovation test)"""
    _fields_ = [("step", C.c_double), ("gamma0", C.c_double), ("iterations", C.c_int32), ("converged", C.c_int32)]


assert C.sizeof(rvio_meas_iter) == 24


def iter_update_model(x0, P0, lin, max_iters, tol, dtype=float):
    """NumPy model of the iterated update (the specification in include/rvio_hip.h): a Gauss-Newton / IEKF loop whose every pass refers to the
    prior (x0, P0).  lin(x, i) -> (H, r, sigma): the family's row model at the state x for pass i.  Returns (x', P', info) with info a dict:
    iterations, steps (one per pass), converged, gamma0, dx.  The gain of every pass is formed against P0; P' is the Joseph form of the final
    pass's gain, symmetrised; the state is always injected from x0.  With max_iters = 1 this is aux_update_model.  No gate (the caller compares
    gamma0).  dtype: np.longdouble runs the linear algebra of the loop in extended precision (the rows and the injection stay float64 — they
    are the family models'), which gives the rounding floor of the float64 loop."""
    x0 = np.asarray(x0, float)
    P = np.asarray(P0, dtype)
    d = P.shape[0]
    dx, x = np.zeros(d, dtype), x0.copy()
    steps, gamma0, conv = [], 0.0, False

    def solve(S, B):   # float64: what aux_update_model calls; else L D L^T by hand (S is symmetric positive definite; numpy.linalg has no longdouble)
        if dtype is float:
            return np.linalg.solve(S, B)
        m = S.shape[0]
        L, D = np.eye(m, dtype=dtype), np.zeros(m, dtype)
        for k in range(m):
            D[k] = S[k, k] - (L[k, :k] ** 2) @ D[:k]
            for i in range(k + 1, m):
                L[i, k] = (S[i, k] - (L[i, :k] * L[k, :k]) @ D[:k]) / D[k]
        Y = np.array(B, dtype, copy=True)
        for k in range(m):
            Y[k] = Y[k] - L[k, :k] @ Y[:k]
        Y = Y / (D[:, None] if Y.ndim == 2 else D)
        for k in range(m - 1, -1, -1):
            Y[k] = Y[k] - L[k + 1:, k] @ Y[k + 1:]
        return Y

    for i in range(int(max_iters)):
        H, r, sigma = lin(x, i)
        H, r, sigma = np.atleast_2d(np.asarray(H, dtype)), np.asarray(r, dtype).reshape(-1), np.asarray(sigma, dtype).reshape(-1)
        m = H.shape[0]
        Hw = H / sigma[:, None]
        vw = r / sigma + Hw @ dx
        T = P @ Hw.T
        S = Hw @ T + np.eye(m, dtype=dtype)
        S = (S + S.T) / 2
        K = solve(S, T.T).T
        if i == 0:
            gamma0 = abs(float(vw @ solve(S, vw)))
        dxn = K @ vw
        steps.append(float(np.max(np.abs(dxn - dx))))
        dx = dxn
        x = inject_state(x0, np.asarray(dx, float))
        conv = steps[-1] < tol
        if conv or i == max_iters - 1:
            IKH = np.eye(d, dtype=dtype) - K @ Hw
            Pn = IKH @ P @ IKH.T + K @ K.T
            return x, (Pn + Pn.T) / 2, {"iterations": i + 1, "steps": steps, "converged": bool(conv), "gamma0": gamma0, "dx": dx}
    raise AssertionError("max_iters >= 1")


# Camera.T_BC0 of config/rvio_euroc.yaml:55-62 (row-major)
_T_BC0 = [0.0148655429818, -0.999880929698, 0.00414029679422, -0.0216401454975,
          0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768,
          -0.0257744366974, 0.00375618835797, 0.999660727178, 0.00981073058949,
          0.0, 0.0, 0.0, 1.0]


def config_euroc(**over):
    """Stock values of config/rvio_euroc.yaml:8-111 (same as C rvio_config_euroc)."""
    c = rvio_config()
    c.imu_rate = 200
    c.sigma_g, c.sigma_wg, c.sigma_a, c.sigma_wa = 1.6968e-04, 1.9393e-05, 2.0e-3, 3.0e-3
    c.gravity = 9.8082
    c.small_angle = 0.001745329
    c.width, c.height = 752, 480
    c.fx, c.fy, c.cx, c.cy = 458.654, 457.296, 367.215, 248.375
    c.k1, c.k2, c.p1, c.p2, c.k3 = -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0
    c.sigma_px, c.sigma_py = 0.002180293, 0.002186767
    for i, v in enumerate(_T_BC0):
        c.T_bc[i] = v
    c.fisheye = 0
    c.n_features, c.max_track_len, c.min_track_len = 200, 15, 3
    c.min_dist, c.qual_lvl = 15, 0.01
    c.block_x, c.block_y = 150, 120
    c.enable_equalizer, c.use_sampson = 1, 1
    c.inlier_thr = 1e-5
    c.ini_thr_angle, c.ini_thr_displ = 0.005, 0.01
    c.ini_enable_alignment = 1
    for k, v in over.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


# BASELINE.json configs (SURVEY.md section 8 size table): name -> overrides
BASELINE_CONFIGS = {
    "A": dict(n_features=200, max_track_len=15),                       # stock EuRoC V1_01
    "B": dict(n_features=200, max_track_len=11),                       # MH_01 200 f / 10 clones (headline)
    "C": dict(n_features=400, max_track_len=21),                       # 400 f / 20 clones
    "D": dict(n_features=800, max_track_len=16, width=1920, height=1080,
              fx=1171.0, fy=1171.0, cx=960.0, cy=540.0, block_x=384, block_y=270),  # 1080p
    "E": dict(n_features=1600, max_track_len=31),                      # 8-GPU 1600 f / 30 clones
}


def config_named(name, **over):
    kw = dict(BASELINE_CONFIGS[name])
    kw.update(over)
    return config_euroc(**kw)


def dims(cfg, n_clones=None):
    """(n_max, d, xdim) for the configured window (or for n_clones)."""
    n = cfg.max_track_len - 1 if n_clones is None else n_clones
    return n, 24 + 6 * n, 26 + 7 * n


def fu(cfg):
    return int(math.ceil(0.5 * cfg.n_features))


def make_tracks(types, lens, meas):
    """Build an rvio_tracks view over numpy arrays (kept alive by the caller)."""
    types = np.ascontiguousarray(types, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    meas = np.ascontiguousarray(meas, dtype=np.float32)
    assert meas.ndim == 3 and meas.shape[2] == 2 and meas.shape[0] >= len(types)
    t = rvio_tracks(len(types), meas.shape[1],
                    types.ctypes.data_as(C.POINTER(C.c_ubyte)),
                    lens.ctypes.data_as(C.POINTER(C.c_int32)),
                    meas.ctypes.data_as(C.POINTER(C.c_float)))
    t._keep = (types, lens, meas)
    return t


def as_imu_array(w, a, t, dt):
    arr = np.zeros(len(t), dtype=IMU_DTYPE)
    arr["w"], arr["a"], arr["t"], arr["dt"] = w, a, t, dt
    return arr


# ---- wire format of a shard's share of the information block (csrc/rvio_dev.h shard_layout: the all-gather payload of rvio_hip_update_local /
# rvio_hip_frame_sharded_dev): [8 counters | S2 tiles | S1 tiles], 16 x 16 tiles of 256 doubles, upper triangle only, S2 only where a type-'2'
# feature can reach.  NumPy mirror for tests and host-side collectives.
def shard_layout(c6, max_len):
    ntq, ntp = (c6 >> 4) + 1, (c6 + 15) >> 4
    hi2 = min(6 * ((max_len + 1) // 2 - 1), c6)
    t2 = min((hi2 - 1) >> 4 if hi2 > 0 else -1, ntp - 1)
    x2 = 1 if ntq - 1 > t2 else 0
    tiles2 = 0 if t2 < 0 else (t2 + 1) * (t2 + 2) // 2 + x2 * (t2 + 1)
    tiles1 = ntp * ntq - ntp * (ntp - 1) // 2
    return dict(ntq=ntq, ntp=ntp, t2=t2, x2=x2, tiles2=tiles2, tiles1=tiles1)


def shard_payload_doubles(c6, max_len):
    L = shard_layout(c6, max_len)
    return 8 + 256 * (L["tiles2"] + L["tiles1"])


def _shard_tiles(L):
    """[(part, pt, qt, offset)] of every carried tile (part 0 = S2, 1 = S1)"""
    out = []
    for pt in range(L["t2"] + 1):
        row = pt * (L["t2"] + 1 + L["x2"]) - pt * (pt - 1) // 2
        for qt in range(pt, L["t2"] + 1):
            out.append((0, pt, qt, 8 + 256 * (row + qt - pt)))
        if L["x2"]:
            out.append((0, pt, L["ntq"] - 1, 8 + 256 * (row + L["t2"] + 1 - pt)))
    for pt in range(L["ntp"]):
        for qt in range(pt, L["ntq"]):
            out.append((1, pt, qt, 8 + 256 * (L["tiles2"] + pt * L["ntq"] - pt * (pt - 1) // 2 + qt - pt)))
    return out


def shard_pack(parts, counters, c6, max_len):
    """parts: (2, rows >= c6, cols >= c6 + 1) full-layout S2, S1 (row p, column q; column c6 = the residual); counters: 8 numbers.
    Returns (payload, live): the wire-format vector and the mask of its entries that carry matrix elements (tile padding excluded)."""
    L = shard_layout(c6, max_len)
    pay = np.zeros(shard_payload_doubles(c6, max_len))
    live = np.zeros(len(pay), bool)
    pay[:8] = counters
    live[:8] = True
    for part, pt, qt, off in _shard_tiles(L):
        r1, c1 = min(16 * pt + 16, c6), min(16 * qt + 16, c6 + 1)
        tile = np.zeros((16, 16))
        mask = np.zeros((16, 16), bool)
        tile[: r1 - 16 * pt, : c1 - 16 * qt] = parts[part][16 * pt: r1, 16 * qt: c1]
        mask[: r1 - 16 * pt, : c1 - 16 * qt] = True
        pay[off: off + 256] = tile.reshape(-1)
        live[off: off + 256] = mask.reshape(-1)
    return pay, live


def shard_unpack(pay, c6, max_len, ld):
    """inverse of shard_pack into full-layout (2, ld, ld) matrices with the lower triangle mirrored from the upper one (the residual column has
    no mirror image), and the 8 counters"""
    L = shard_layout(c6, max_len)
    parts = np.zeros((2, ld, ld))
    for part, pt, qt, off in _shard_tiles(L):
        r1, c1 = min(16 * pt + 16, c6), min(16 * qt + 16, c6 + 1)
        parts[part][16 * pt: r1, 16 * qt: c1] = np.asarray(pay[off: off + 256]).reshape(16, 16)[: r1 - 16 * pt, : c1 - 16 * qt]
    for part in range(2):
        a = parts[part][:c6, :c6]
        iu = np.triu_indices(c6, 1)
        # tiles strictly above the diagonal tile row carry both triangles of nothing: only elements whose TILE lies on or above the diagonal are valid
        valid = (iu[1] >> 4) >= (iu[0] >> 4)
        a[(iu[1][valid], iu[0][valid])] = a[(iu[0][valid], iu[1][valid])]
    return parts, np.array(pay[:8])
