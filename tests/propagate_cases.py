"""Inputs and truth shared by the propagate edge tests (test infrastructure): start states from recorded direct-track sequences, IMU batches at
the shapes PreIntegrator::propagate's device forms can go wrong at, the oracle's result, a fresh np.longdouble restatement of the recursion on the
24 x 24 head, and the conditions that make a case worth a launch.

The device (csrc/filter_kernels2.hip, propagate_body) cuts the batch into chunks of 16 samples (8 in propagate_kernel3b), composes each chunk's
transition as suffix products and carries the serial chain through LDS.  With m = 10 and dt = 0.005 on every sample — all the recorded frames
have — a dt picked across a chunk boundary, a Dt not carried, a Q_s paired with the wrong S_s or a wrong nSmallAngle branch cannot be seen.  So:

  irregular(m)   dt = 0.005 * {0, 0.6, 1, 1, 1.4, 2, 3} per sample (duplicates, jitter, dropped samples), about m / 5 samples slower than the stock
                 small_angle after the bias is removed (scattered, the chunks' first and last samples among them), one sample with w == bg exactly;
  branch(m)      small_angle = 0.5, dt = 0.05, |w - bg| alternating 0.4 (in the branch) / 0.6 (out of it): settings at which the two branches differ
                 by 1e-6 and more (at stock settings they agree to 1e-13: a wrong branch would pass every test).

Each case is checked on the CPU, from the oracle alone, before it is worth sending to the device (conditions(): swapping the dt of the two samples
on either side of every chunk boundary, or forcing the other branch, must move the oracle's result by >= 1000 x the bar the case is checked at).
"""
import functools

import numpy as np

import oracle as O
import scenarios as S
from test_gpu_filter import X_TOL, p_close          # the project's state bar and its P norm

abi, rv = O.abi, O.rv

M_EDGES = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 65)
DT0 = 0.005
DT_MULT = (0.0, 0.6, 1.0, 1.0, 1.4, 2.0, 3.0)
# max_ij |dP_ij| / sqrt(P_ii P_jj) against the oracle, head and head-by-clone cross block.  Measured on the MI355X over every propagate-only case of
# tests/test_gpu_propagate_edges.py (plain and batch forms): worst 2.97e-15 (profiles/propagate_edges.md) — the oracle's own distance to the
# np.longdouble recursion is 2.66e-15 (tests/test_propagate_cases.py), so the device sits on the reference's floor.  The bar: 10 x that worst value,
# rounded up to a power of ten; the factor covers the reassociation of the batch forms from run to run.  It may not exceed 1e-8.
P_NORM_BAR = 1e-13
assert P_NORM_BAR <= 1e-8
SENSITIVITY = 1000.0          # a case must react to the error it is there for by this many bars
BOUNDARIES = (8, 16, 32)      # first sample of a new chunk: 7|8 (chunks of 8), 15|16 and 31|32 (chunks of 16; 8-chunks end there too)
MID_ML = 14                   # 13 clones, 6n = 78: propagate_chol_kernel<3> (6n_max in 65..96)
STATES = ("empty", "window10", "mid", "long")


def long_ml():
    import test_gpu_windows as TW
    return max(w[0] for w in TW.WINDOWS)


@functools.lru_cache(maxsize=None)
def config(state, small_angle=None):
    """the cfg of a start state; small_angle: the same cfg with another nSmallAngle (the state does not depend on it)"""
    kw = {} if small_angle is None else dict(small_angle=small_angle)
    if state in ("empty", "window10"):
        return abi.config_named("B", enable_equalizer=0, **kw)
    import test_gpu_windows as TW
    return TW.window_cfg(MID_ML if state == "mid" else long_ml(), **kw)


def n_clones(state):
    return {"empty": 0, "window10": 10, "mid": MID_ML - 1, "long": long_ml() - 1}[state]


@functools.lru_cache(maxsize=None)
def recorded(state):
    """the fewest frames that fill the window: record f starts with f - 1 clones (the first image augments nothing)"""
    cfg = config("window10" if state == "empty" else state)
    n = n_clones("window10" if state == "empty" else state)
    assert n == cfg.max_track_len - 1
    return S.record_sequence(cfg, n_frames=n + 2, duration=6.0)


def frame_record(state):
    """the recorded frame that starts on the full window (it has an update)"""
    r = recorded(state)[1][-1]
    assert (len(r["x0"]) - 26) // 7 == n_clones(state) and r["did_update"]
    return r


@functools.lru_cache(maxsize=None)
def _state(state):
    if state == "empty":
        r = recorded("window10")[1][0]
    else:
        r = frame_record(state)
    x, P = r["x0"], r["P0"]
    n = n_clones(state)
    assert len(x) == 26 + 7 * n and P.shape == (24 + 6 * n, 24 + 6 * n)
    if state == "long":
        assert 6 * n > 144          # propagate_kernel3b stages the clone cross-columns in two tiles
    if state == "mid":
        assert 65 <= 6 * n <= 96
    return x, P


def state(name):
    x, P = _state(name)
    return x.copy(), P.copy()


@functools.lru_cache(maxsize=None)
def _imu_all(seed):
    return rv.synth.SynthSequence(config("window10"), duration=8.0, seed=seed).imu_all()


def _stretch(m, seed):
    """m consecutive samples of a moving stretch"""
    a = 600 + 53 * seed
    imu = _imu_all(seed % 3)[a: a + m].copy()
    assert len(imu) == m
    return imu


@functools.lru_cache(maxsize=None)
def _irregular(m, seed, bg):
    rng = np.random.default_rng([7, m, seed])
    imu = _stretch(m, seed)
    bg = np.array(bg)
    while True:
        dt = DT0 * rng.choice(DT_MULT, size=m)
        if dt.sum() > 0 and all(dt[b - 1] != dt[b] for b in BOUNDARIES if b < m):
            break
    imu["dt"] = dt
    # slower than the stock small_angle: the chunks' edges first, the rest anywhere
    edges = [p for p in (0, 7, 8, 15, 16, 31, 32, m - 1) if p < m]
    n_slow = (m + 2) // 5
    pick = list(rng.permutation(edges)[: (n_slow + 1) // 2]) if n_slow else []
    rest = [p for p in rng.permutation(m) if p not in pick]
    slow = (pick + rest)[:n_slow]
    for p in slow:
        imu["w"][p] = bg + rng.normal(0.0, 3e-4, 3)
    zero = int(rng.integers(m)) if m > 1 else int(seed % 2 == 0) - 1      # (m = 1: every other seed, so that the lone sample also runs the general branch)
    if zero >= 0:
        imu["w"][zero] = bg
    return imu, tuple(sorted(int(p) for p in slow)), zero


def irregular(m, x, seed=0):
    """(imu, slow positions, position of the w == bg sample or -1)"""
    imu, slow, zero = _irregular(m, seed, tuple(float(v) for v in x[20:23]))
    return imu.copy(), slow, zero


BRANCH_SMALL_ANGLE, BRANCH_DT = 0.5, 0.05


@functools.lru_cache(maxsize=None)
def _branch(m, seed, bg):
    rng = np.random.default_rng([11, m, seed])
    imu = _stretch(m, seed)
    imu["dt"] = BRANCH_DT
    for s in range(m):
        d = rng.normal(size=3)
        imu["w"][s] = np.array(bg) + (0.4 if (s + seed) % 2 == 0 else 0.6) * d / np.linalg.norm(d)
    return imu


def branch(m, x, seed=0):
    return _branch(m, seed, tuple(float(v) for v in x[20:23])).copy()


def batch(kind, m, x, seed=0):
    return irregular(m, x, seed)[0] if kind == "irregular" else branch(m, x, seed)


def case_cfg(state_name, kind):
    return config(state_name, BRANCH_SMALL_ANGLE if kind == "branch" else None)


@functools.lru_cache(maxsize=None)
def case(state_name, kind, m, seed=0):
    """(cfg, x, P, imu, (x1, P1) of the oracle), computed once per session; the arrays are shared: do not write to them"""
    x, P = _state(state_name)
    cfg = case_cfg(state_name, kind)
    imu = batch(kind, m, x, seed)
    return cfg, x, P, imu, O.propagate(cfg, x, P, imu)


# ------------------------------------------------------------------------------------------------ norms
def p_proj(Pa, Pb):
    return float(np.max(np.abs(Pa - Pb)) / np.max(np.abs(Pb)))


def p_norm(Pa, Pb):
    """max_ij |dP_ij| / sqrt(P_ii P_jj) over the head and the head-by-clone cross block, with Pb's diagonal (entries with a zero variance on
    either side — the relative pose behind composition, the empty window's — are left to the project norm)"""
    d = np.sqrt(np.maximum(np.diag(Pb), 0.0))
    sc = np.outer(d, d)
    E = np.abs(np.asarray(Pa) - Pb)
    ok = sc > 0
    ok[24:, 24:] = False
    return float(np.max(E[ok] / sc[ok])) if ok.any() else 0.0


# ------------------------------------------------------------------------------------------------ the recursion in np.longdouble
LD = np.longdouble


def _skew_ld(v):
    z = LD(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=LD)


def _q2r_ld(q):
    """JPL: I - 2 w [q]x + 2 [q]x^2"""
    q = np.asarray(q, LD)              # (not normalised: the initial state's qk is all zero and stands for the identity, as QuatToRot has it)
    qx = _skew_ld(q[:3])
    return np.eye(3, dtype=LD) - LD(2) * q[3] * qx + LD(2) * (qx @ qx)


def _r2q_ld(R):
    """RotToQuat, the four-branch form, normalised, w >= 0 (Rk is not exactly orthonormal behind the second-order small-angle dR: the quaternion
    is what the state keeps, so it is what is compared)"""
    d = [R[0, 0], R[1, 1], R[2, 2]]
    T = d[0] + d[1] + d[2]
    q = np.zeros(4, LD)
    big = [i for i in range(3) if d[i] > T and all(d[i] > d[j] for j in range(3) if j != i)]
    if big:
        i = big[0]
        j, k = (i + 1) % 3, (i + 2) % 3
        q[i] = np.sqrt((1 + 2 * d[i] - T) / 4)
        s = 1 / (4 * q[i])
        q[j], q[k], q[3] = s * (R[i, j] + R[j, i]), s * (R[i, k] + R[k, i]), s * (R[j, k] - R[k, j])
    else:
        q[3] = np.sqrt((1 + T) / 4)
        s = 1 / (4 * q[3])
        q[0], q[1], q[2] = s * (R[1, 2] - R[2, 1]), s * (R[2, 0] - R[0, 2]), s * (R[0, 1] - R[1, 0])
    q = q / np.sqrt(q @ q)
    return -q if q[3] < 0 else q


def longdouble_model(cfg, x, P24, imu):
    """PreIntegrator::propagate's sample loop on the state head and the 24 x 24 head of P in np.longdouble: Phi = I + dt F,
    P <- Phi P Phi^T + dt G Sig G^T, and the state half.  Returns (Rk, pk, vk, P) as longdouble arrays."""
    x = np.asarray(x[:26], LD)
    P = np.array(np.asarray(P24)[:24, :24], dtype=LD)
    gR, vR, bg, ba = x[7:10].copy(), x[17:20].copy(), x[20:23], x[23:26]
    Rk, pk, vk, gk = _q2r_ld(x[10:14]), x[14:17].copy(), vR.copy(), gR.copy()
    dp, dv, Dt = np.zeros(3, LD), np.zeros(3, LD), LD(0)
    I = np.eye(3, dtype=LD)
    g = LD(cfg.gravity)
    Sig = np.diag(np.repeat(np.array([cfg.sigma_g, cfg.sigma_wg, cfg.sigma_a, cfg.sigma_wa], LD) ** 2, 3))
    small_angle = LD(cfg.small_angle)
    for u in imu:
        dt = LD(u["dt"])
        Dt = Dt + dt
        w, a = np.asarray(u["w"], LD) - bg, np.asarray(u["a"], LD) - ba
        wx, vx = _skew_ld(w), _skew_ld(vk)
        F, G = np.zeros((24, 24), LD), np.zeros((24, 12), LD)
        F[9:12, 9:12], F[9:12, 18:21] = -wx, -I
        F[12:15, 9:12], F[12:15, 15:18] = -Rk.T @ vx, Rk.T
        F[15:18, 6:9], F[15:18, 9:12], F[15:18, 15:18], F[15:18, 18:21], F[15:18, 21:24] = -g * Rk, -g * _skew_ld(gk), -wx, -vx, -I
        G[9:12, 0:3], G[15:18, 0:3], G[15:18, 6:9], G[18:21, 3:6], G[21:24, 9:12] = -I, -vx, -I, I, I
        Phi = np.eye(24, dtype=LD) + dt * F
        P = Phi @ P @ Phi.T + (dt * G) @ Sig @ G.T
        w1 = np.sqrt(w @ w)
        wdt = w1 * dt
        wx2 = wx @ wx
        if w1 < small_angle:
            dR = I - dt * wx + (dt ** 2 / 2) * wx2
            f1, f2, f3, f4 = -dt ** 3 / 3, dt ** 4 / 8, -dt ** 2 / 2, dt ** 3 / 6
        else:
            c, s = np.cos(wdt), np.sin(wdt)
            dR = I - (s / w1) * wx + ((1 - c) / w1 ** 2) * wx2
            f1 = (wdt * c - s) / w1 ** 3
            f2 = LD(0.5) * (wdt * wdt - 2 * c - 2 * wdt * s + 2) / w1 ** 4
            f3 = (c - 1) / w1 ** 2
            f4 = (wdt - s) / w1 ** 3
        Rk = dR @ Rk
        dp = dp + dv * dt
        dp = dp + Rk.T @ ((LD(0.5) * dt ** 2 * I + f1 * wx + f2 * wx2) @ a)
        dv = dv + Rk.T @ ((dt * I + f3 * wx + f4 * wx2) @ a)
        pk = vR * Dt - LD(0.5) * g * gR * Dt ** 2 + dp
        vk = Rk @ (vR - g * gR * Dt + dv)
        gk = Rk @ gR
        gk = gk / np.sqrt(gk @ gk)
    return Rk, pk, vk, LD(0.5) * (P + P.T)


def oracle_vs_longdouble(state_name, kind, m, seed=0):
    """(state delta, project norm, normalised norm) of the oracle against the longdouble model on the head: the reference's own rounding floor"""
    cfg, x, P, imu, (x1, P1) = case(state_name, kind, m, seed)
    Rk, pk, vk, Pl = longdouble_model(cfg, x, P, imu)
    q1 = np.asarray(x1[10:14], LD)
    dq = np.max(np.abs((-q1 if q1[3] < 0 else q1) - _r2q_ld(Rk)))
    dx = max(float(dq), float(np.max(np.abs(x1[14:17] - pk))), float(np.max(np.abs(x1[17:20] - vk))))
    Pl = np.asarray(Pl, float)
    return dx, p_proj(P1[:24, :24], Pl), p_norm(P1[:24, :24], Pl)


# ------------------------------------------------------------------------------------------------ can the case fail?
def _moved(a, b):
    """(state delta, normalised P) between two oracle results"""
    return S.state_delta(a[0], b[0]), p_norm(a[1], b[1])


def reacts(d):
    return d[0] >= SENSITIVITY * X_TOL or d[1] >= SENSITIVITY * P_NORM_BAR


@functools.lru_cache(maxsize=None)
def conditions(state_name, kind, m, seed=0):
    """{what: (state delta, normalised P)} of the oracle under the errors the case is there for; asserts that each is >= 1000 bars"""
    cfg, x, P, imu, truth = case(state_name, kind, m, seed)
    assert np.all(np.isfinite(truth[0])) and np.all(np.isfinite(truth[1])), (state_name, kind, m, seed)
    out = {}
    if kind == "irregular":
        for b in BOUNDARIES:
            if b < m:
                sw = imu.copy()
                assert sw["dt"][b - 1] != sw["dt"][b]
                sw["dt"][[b - 1, b]] = sw["dt"][[b, b - 1]]
                out["dt %d|%d" % (b - 1, b)] = _moved(O.propagate(cfg, x, P, sw), truth)
    else:
        d = _moved(O.propagate(config(state_name, 1e-12), x, P, imu), truth)
        assert d[0] >= SENSITIVITY * X_TOL, (state_name, m, seed, d)      # in the state itself: dR and f1..f4 are the branch
        out["branch"] = d
    for what, d in out.items():
        assert reacts(d), (state_name, kind, m, seed, what, d)
    return out
