"""Cases for the landmark-covariance tests (tests/test_landmark_cov_model.py on the CPU, tests/test_gpu_landmark_cov.py on the device): a
propagated state with a full clone window per max_track_len, hand-over tables whose tracks are consistent with that state's relative-pose
chain, a Gauss-Newton triangulation in NumPy, and the error measure the covariances are held to.  Built once per window and shared."""
import functools

import numpy as np

import oracle as O
import scenarios as S

abi, rv = O.abi, O.rv
WINDOWS = (3, 10, 32)        # max_track_len: n = 2 (L = 2 and 3: the smallest chain), 9 (stock-sized), 31 (span 186 + 6 columns: the LDS edge)
BAR = 1e-11                  # the project's bar for a device covariance against the extended-precision twin
FLOOR_BAR = 1e-12            # ... provided the float64 model's own floor against the twin stays below this


def cov_err(Cm, C_true):
    """max |C - C_true|_ij / sqrt(C_ii C_jj): every entry on the scale of its correlation"""
    Ct = np.asarray(C_true, np.longdouble)
    d = np.sqrt(np.diag(Ct))
    return float(np.max(np.abs(np.asarray(Cm, np.longdouble) - Ct) / np.outer(d, d)))


def project_track(cfg, x, ftype, L, pc1, noise=None):
    """the L normalised observations of the point pc1 (first camera frame) through the relative-pose chain of x (Updater.cc:125-141)"""
    n = (len(x) - 26) // 7
    T = np.array(list(cfg.T_bc)).reshape(4, 4)
    Ric, tic = T[:3, :3], T[:3, 3]
    Rci = Ric.T
    nph = L - 1
    c0 = n - nph if ftype == "1" else 0
    X = Ric @ pc1 + tic
    obs = [pc1[:2] / pc1[2]]
    for i in range(nph):
        a = 26 + 7 * (c0 + i)
        X = abi.quat_to_rot(x[a: a + 4]) @ (X - x[a + 4: a + 7])
        pc = Rci @ (X - tic)
        obs.append(pc[:2] / pc[2])
    obs = np.array(obs)
    return obs if noise is None else obs + noise


def make_tracks(cfg, x, spec, seed=0, noise=True):
    """hand-over tables (types, lens, meas) of the tracks spec = [(type, L), ...] seen from the state x: a random point 2 .. 8 m in front of
    each track's first camera, projected through the state's own chain, plus sigma_im noise (rv.synth.worst_case_tracks with the track
    kinds chosen by the caller)"""
    rng = np.random.default_rng(4321 + seed)
    sig = abi.landmark_sigma(cfg)
    types, lens = np.zeros(len(spec), np.uint8), np.zeros(len(spec), np.int32)
    meas = np.zeros((len(spec), cfg.max_track_len, 2), np.float32)
    for f, (ty, L) in enumerate(spec):
        depth = rng.uniform(2.0, 8.0)
        pc1 = np.array([rng.uniform(-0.5, 0.5) * depth, rng.uniform(-0.35, 0.35) * depth, depth])
        nz = sig * rng.standard_normal((L, 2))
        types[f], lens[f] = ord(ty), L
        meas[f, :L] = project_track(cfg, x, ty, L, pc1, nz if noise else None).astype(np.float32)
    return types, lens, meas


def spec_for(max_len, n_feat):
    """track kinds of a hand-over table of n_feat features at a full window of max_len - 1 clones: every second one type '2' at full length,
    the others type '1' running through every length 2 .. max_len (L = 2: one clone, the shortest chain)"""
    spec = []
    for f in range(n_feat):
        spec.append(("2", max_len) if f % 2 == 0 else ("1", 2 + (f // 2) % (max_len - 1)))
    return spec


@functools.lru_cache(maxsize=None)
def window_case(max_len, n_feat=24):
    """(cfg, x1, P1, types, lens, meas): the propagated state of an oracle sequence at the first frame with a full window of max_len - 1
    clones, and a hand-over table of both track types consistent with it"""
    cfg = abi.config_named("B", enable_equalizer=0, max_track_len=max_len, n_features=60 if max_len > 11 else 200)
    _, recs = S.record_sequence(cfg, n_frames=max_len + 3)
    r = recs[-1]
    assert (len(r["x1"]) - 26) // 7 == max_len - 1
    x1, P1 = r["x1"].copy(), r["P1"].copy()
    types, lens, meas = make_tracks(cfg, x1, spec_for(max_len, n_feat), seed=max_len)
    for a in (x1, P1, types, lens, meas):
        a.setflags(write=False)
    return cfg, x1, P1, types, lens, meas


def residuals(cfg, x, ftype, L, meas, pf):
    """r = z - h(theta, x) of all L observations (2L), in float64"""
    phi, psi, rho = pf
    e = np.array([np.cos(phi) * np.sin(psi), np.sin(phi), np.cos(phi) * np.cos(psi)])
    return (np.asarray(meas[:L], float) - project_track(cfg, x, ftype, L, e / rho)).ravel()


def solve_theta(cfg, x, ftype, L, meas, pf0, iters=8):
    """theta = argmin |z - h(theta, x)|^2 by Gauss-Newton from pf0 with the model's own Hf"""
    pf = np.array(pf0, float)
    for _ in range(iters):
        Hf = abi.landmark_cov_model(cfg, x, None, ftype, L, meas, pf, hf_only=True)["Hf"]
        dp = np.linalg.solve(Hf.T @ Hf, Hf.T @ residuals(cfg, x, ftype, L, meas, pf))
        pf = pf + dp
        if np.max(np.abs(dp)) < 1e-10:          # (quadratic convergence: the step behind this one is below 1e-19)
            break
    return pf


def point_of(cfg, x, ftype, L, pf):
    """(p_r, p_w) of theta at the state x, as the record defines them"""
    m = abi.landmark_cov_model(cfg, x, None, ftype, L, None, pf, hf_only=True)
    return m["p_r"], m["p_w"]
