"""Inputs shared by the map-landmark tests (test infrastructure): the window states of tests/aux_update_cases.py (plus a 32-clone state grown from
the longest one, for the CPU model only: no handle holds more than 31 clones), two calibrations (radial-tangential and fisheye, both with a
camera-IMU transform that is far from the identity), and observations of world points placed a known way in the camera of the image `age` back:
in front of it with a small residual ("good"), with a gross residual ("outlier"), or behind it ("behind")."""
import numpy as np

import fix_past_cases as FP

abi, A, K, F = FP.abi, FP.A, FP.K, FP.F
WINDOWS = (0, 1, 3, 10, 31, 32)
GPU_WINDOWS = (0, 1, 3, 10, 31)          # what a handle can hold (max_track_len = 32: 31 clones)
SIGMA = 0.004                            # normalised units: about two pixels at the stock focal length
GOOD, OUTLIER, BEHIND = "good", "outlier", "behind"


def state(n):
    """(x, P) with n clones; n = 32: the 31-clone state with one more (oldest) clone in front, P grown by an independent 6 x 6 block"""
    if n <= 31:
        return A.window_state(n)
    x31, P31 = A.window_state(31)
    rng = np.random.default_rng(3232)
    q = np.concatenate([0.02 * rng.standard_normal(3), [1.0]])
    x = np.concatenate([x31[:26], q / np.linalg.norm(q), 0.05 * rng.standard_normal(3), x31[26:]])
    d = 24 + 6 * 32
    P = np.zeros((d, d))
    old = np.r_[0:24, 30:d]
    P[np.ix_(old, old)] = P31
    P[24:30, 24:30] = 1e-4 * np.eye(6)
    return x, P


def ages(n):
    return FP.ages(n)


def gpu_ages(n):
    """both sides of 64 and of 128 columns that are not zero (6 + 6 a), the ends and the first step"""
    return sorted({a for a in (0, 1, 9, 10, 11, 20, 21, 22, n) if a <= n})


def calibrations():
    """name -> rvio_calibration: the stock radial-tangential camera and a fisheye one with another extrinsic; fx == fy in both, so that a PIXELS
    call and a NORMALISED twin can carry the same sigmas"""
    cfg = A.long_config()
    rt = abi.calibration_from_config(cfg)
    rt.fy = rt.fx
    fe = abi.calibration_from_config(cfg)
    fe.fisheye, fe.fx, fe.fy, fe.cx, fe.cy = 1, 380.0, 380.0, 370.0, 240.0
    fe.k1, fe.k2, fe.p1, fe.p2, fe.k3 = -0.013, 0.021, -0.008, 0.0015, 0.0
    R = abi.quat_to_rot(F.rot_quat(np.array([0.4, -0.7, 0.5])))
    T = np.eye(4)
    T[0:3, 0:3], T[0:3, 3] = R, (0.07, -0.03, 0.11)
    for i, v in enumerate(T.reshape(-1)):
        fe.T_bc[i] = float(v)
    return {"radtan": rt, "fisheye": fe}


def _world_of(cal, x, age, pC):
    """the world point that lies at pC in the camera of the image `age` back"""
    Rci, tci = abi._map_cam(cal)
    Ach, t = abi._fix_past_chain(x, age)
    w = Ach[age] @ (Rci.T @ (np.asarray(pC, float) - tci)) + t[age]
    return abi.quat_to_rot(x[0:4]).T @ (w - x[4:7])


def observations(cal, x, age, kinds, seed=0, sigma=SIGMA):
    """one (p_w, uv, sigma) per entry of `kinds`, NORMALISED units: GOOD — 2 .. 6 m in front, the residual 0.5 sigma per axis at most; OUTLIER —
    the same with a residual of 0.3 (75 sigma); BEHIND — 3 m behind the camera"""
    rng = np.random.default_rng(477 + seed)
    out = []
    for kind in kinds:
        zc = rng.uniform(2.0, 6.0) * (-1.0 if kind == BEHIND else 1.0)
        hn = rng.uniform(-0.4, 0.4, 2)
        pC = np.array([hn[0] * zc, hn[1] * zc, zc])
        off = rng.uniform(-0.5, 0.5, 2) * sigma
        if kind == OUTLIER:
            off = 0.3 * np.array([1.0, -1.0])[rng.integers(0, 2, 2)]
        out.append((_world_of(cal, x, age, pC), hn + off, sigma))
    return out


def pixel_observations(cal, x, age, k, seed=0, sigma_px=1.5):
    """k (p_w, uv, sigma) in PIXELS: points in front of the camera, the pixel at the pinhole image of the point plus up to 3 px (the distortion
    is left out on purpose: the residual then holds it, and nothing is gated in the pixel tests)"""
    rng = np.random.default_rng(577 + seed)
    out = []
    for p_w, uv, _ in observations(cal, x, age, [GOOD] * k, seed):
        px = np.array([cal.fx * uv[0] + cal.cx, cal.fy * uv[1] + cal.cy]) + rng.uniform(-3, 3, 2)
        out.append((p_w, px, sigma_px))
    return out


GATE_KINDS = (GOOD, GOOD, OUTLIER, GOOD, BEHIND, GOOD, OUTLIER, GOOD)
GATE_STATUS = (0, 0, 1, 0, 2, 0, 1, 0)
GATE_N, GATE_AGE = 10, 4


def gate_case():
    """(cal, x, P, age, observations): a stack of 8 with 2 gross outliers and 1 point behind the camera"""
    cal = calibrations()["radtan"]
    x, P = state(GATE_N)
    return cal, x, P, GATE_AGE, observations(cal, x, GATE_AGE, GATE_KINDS, seed=31)


def row_cases(windows=WINDOWS, age_fn=ages, counts=(1, 2, 3, 8)):
    """(n, age, count, calibration name, seed) of every rows case"""
    out = []
    for n in windows:
        for ai, a in enumerate(age_fn(n)):
            for ci, k in enumerate(counts):
                out.append((n, a, k, ("radtan", "fisheye")[(ai + ci) % 2], 100 * n + 10 * a + k))
    return out


def replaced_outside(x, age, seed=0):
    """the state with entries 7 - 25 (gravity, qk, pk, v, bg, ba: columns 6 - 23) and every clone older than n - age replaced by other valid
    values"""
    rng = np.random.default_rng(677 + seed)
    x = np.array(x, float)
    n = (len(x) - 26) // 7

    def quat():
        q = rng.standard_normal(4)
        return q / np.linalg.norm(q)
    g = rng.standard_normal(3)
    x[7:10] = g / np.linalg.norm(g)
    x[10:14], x[14:17] = quat(), 0.1 * rng.standard_normal(3)
    x[17:26] = 0.1 * rng.standard_normal(9)
    for i in range(0, n - age):
        x[26 + 7 * i: 30 + 7 * i], x[30 + 7 * i: 33 + 7 * i] = quat(), 0.1 * rng.standard_normal(3)
    return x
