"""Fixed cases for the tests of the per-feature stage of the update (tests/test_feature_update_model.py on the CPU,
tests/test_gpu_feature_stage.py on the device): per window one track of every (type, length) the window accepts on a recorded full window, the
zero-parallax tracks that take the N = 2 branch, and hand-built tracks for every branch of the LM loop — with the measures, the bars and the
conditions a case has to meet (stable branch decisions under last-bit noise, gamma away from its threshold, |Hf[:, 2]| away from 1e-4, the
float32 residual of the twin equal to the oracle's, a triple that does not hang on the last bit of the state or of the 3 x 3 solve).  Everything
is seeded; a case that fails a condition is REPLACED here (KIND_DRAW / STILL_DRAW / LM_DRAW name the draw that is taken), never skipped at run
time.  Built once per window and shared."""
import functools

import numpy as np

import landmark_cov_cases as K
import oracle as O

abi, rv = O.abi, O.rv

# max_track_len: 3 (L = 2 and 3 only), 10 (stock), 16 (the last window of geom4_kernel; nPh = 15: the last prefix-scan chain), 17 (nPh = 16: the
# serial chain; L = 17: the unpacked LM sums; batch handles without geom4_kernel), 22 (6n = 126: 128-thread workgroups, rr up to 41), 32 (rr up
# to 61 on 256 threads)
WINDOWS = (3, 10, 16, 17, 22, 32)
LM_WINDOWS = (10, 17)        # the hand-built LM tracks: geom4_kernel's loop on a batch handle at 10, feat_build_kernel<4>'s own at 17
DRAWS = 16                   # last-bit draws per case (section "conditions")

# ---- bars.  gamma and the share: the device is held to 16 x the float64 model's floor against the np.longdouble twin (same conditioning, a
# different but equally backward-stable algorithm).  The floors — one float64 evaluation per case at the oracle's triple, printed by
# tests/test_feature_update_model.py::test_float64_floor_against_the_twin, kept in the docstring of tests/test_gpu_feature_stage.py — do not
# follow cond(S) (below 8 on all but a few cases) but the condition of what the projection takes out: where cond(Hf) is large, a column of Hx or
# the residual lies almost inside span(Hf) and what is left of it carries the rounding of the whole.  So the bars take the form the floors
# scale with, K 2^-52 cond(Hf), K = 16 x the worst measured ratio floor / (2^-52 cond(Hf)) over all cases, rounded up (floors_of); never above
# what the suite held before.
SHARE_SUITE = 1e-9
GAMMA_RTOL_SUITE, PF_RTOL, PF_ATOL = 1e-7, 1e-8, 1e-10      # what the suite held before (tests/test_gpu_filter.py::test_update_parity)
# the triple of one device form against another's: 16 x the worst move of the oracle's own triple under the last-bit draws of check_conditions, in
# the scale-free form |dpf| / (|pf| + 1): 3.9e-4 (the reject-then-accept LM track of window 10; 2.7e-5 on the kinds of window 32 — one float32 ulp
# on an observation moves a triangulated depth that far), rounded up.  Both forms are also held to the oracle at PF_RTOL, which binds long before.
PF_FORM_BAR = 8e-3

def kinds(max_len):
    """every (type, L) the window accepts.  Type '2' starts at L = 3: at L = 2 it keeps one observation and no degree of freedom.  No tracker
    emits it (type '2' is a track that reached max_track_len >= 3), the reference reads its chi^2 table at index -1 there, and so would the
    device (kChi2Dev[rr - 1] at rr = 0 in feat_build_body): a read outside the table, which is why no test hands it to a GPU."""
    return [("1", L) for L in range(2, max_len + 1)] + [("2", L) for L in range(3, max_len + 1)]


# Which draw of the seeded generator each case takes, in the order of kinds(max_len): the first draw whose track meets check_conditions (a
# track whose LM loop ends in the float32 noise floor of its cost — most tracks with pixel noise — exits at an iteration that one float32
# ulp on an observation moves, and is replaced by the next draw).  Found on the CPU with tools of this module (find_draws); the CPU test
# asserts the conditions on every one.
KIND_DRAW = {
    3: (5, 14, 47),
    10: (0, 1, 0, 0, 3, 0, 0, 0, 3, 184, 32, 8, 0, 0, 0, 5, 3),
    16: (0, 0, 0, 1, 0, 0, 16, 6, 0, 6, 26, 2, 2, 1, 4, 208, 23, 0, 0, 7, 1, 3, 0, 1, 5, 10, 12, 4, 13),
    17: (0, 0, 0, 3, 0, 0, 9, 6, 4, 2, 4, 5, 8, 9, 12, 14, 74, 16, 0, 1, 2, 1, 1, 1, 0, 1, 10, 4, 3, 1, 3),
    22: (0, 2, 5, 6, 6, 1, 0, 4, 0, 1, 0, 2, 0, 2, 1, 0, 0, 0, 5, 0, 2, 9, 8, 4, 3, 0, 1, 1, 4, 0, 2, 2, 0, 5, 2, 4, 0, 3, 0, 0, 1),
    32: (0, 0, 0, 4, 0, 8, 8, 10, 2, 0, 20, 0, 3, 1, 1, 3, 2, 0, 2, 0, 2, 0, 0, 0, 7, 0, 2, 0, 0, 8, 0, 9, 40, 8, 1, 0, 0, 0, 0, 3, 1, 1, 9, 5, 22, 1, 7, 1, 9, 1, 1, 1, 1, 8, 0, 1, 5, 0, 0, 3, 0),
}
STILL_DRAW = {
    10: (2,),
    17: (2, 0, 0),
}


def _draw_seed(max_len, ty, L, k, extra=0):
    return 100000 * k + 1000 * max_len + 40 * (ty == "2") + L + 7919 * extra


# Pixel noise of the kind cases, in units of sigma_im.  At full size a track cannot meet check_conditions: its cost ends in the noise floor that the
# float32 rounding of the predicted pixel leaves (d cost = 2 e de / sigma^2 ~ 1e-5 at e ~ sigma, against the loop's 1e-6 test), the loop leaves
# at the first chance rise of the cost, and one float32 ulp on an observation moves that iteration — measured: no draw of 4000 is stable for
# most kinds of window 10.  At 3e-4 sigma (some twenty float32 ulps of an observation) the floor is below 1e-7 and the loop leaves by its own
# test; gamma is then ~1e-7 ndof and such a feature passes the gate.  The refusing side of the gate is reached all the same: on the long windows
# (22, 32) the first step from rho = 0 overshoots on every fourth long track, its cost is compared with itself in the next iteration, the step from
# there has dp[2] < 1e-6 and the loop leaves at iteration 2 with a cost of 1e6 (the reference's own behaviour; gamma 70 .. 3e6) — and by the LM
# classes below.
KIND_NOISE = 3e-4


def _one_track(cfg, x, max_len, ty, L, k, extra=0):
    """draw k of the track of kind (ty, L): a point 2 .. 8 m in front of the first camera through the state's own chain (K.project_track), the
    observations moved by KIND_NOISE sigma_im"""
    rng = np.random.default_rng(_draw_seed(max_len, ty, L, k, extra))
    depth = rng.uniform(2.0, 8.0)
    pc1 = np.array([rng.uniform(-0.5, 0.5) * depth, rng.uniform(-0.35, 0.35) * depth, depth])
    meas = np.zeros((max_len, 2), np.float32)
    meas[:L] = K.project_track(cfg, x, ty, L, pc1, KIND_NOISE * abi.landmark_sigma(cfg) * rng.standard_normal((L, 2)))
    return meas


@functools.lru_cache(maxsize=None)
def window_state(max_len):
    """(cfg, x1, P1): the propagated state of the landmark-covariance cases at the first frame with a full window of max_len - 1 clones"""
    return K.window_case(max_len)[:3]


@functools.lru_cache(maxsize=None)
def kind_cases(max_len):
    """(cfg, x1, P1, types, lens, meas): one noisy track of every kind of `kinds(max_len)` seen from the recorded window"""
    cfg, x1, P1 = window_state(max_len)
    ks = kinds(max_len)
    types, lens, meas = np.zeros(len(ks), np.uint8), np.zeros(len(ks), np.int32), np.zeros((len(ks), max_len, 2), np.float32)
    for f, (ty, L) in enumerate(ks):
        types[f], lens[f], meas[f] = ord(ty), L, _one_track(cfg, x1, max_len, ty, L, KIND_DRAW[max_len][f])
    for a in (types, lens, meas):
        a.setflags(write=False)
    return cfg, x1, P1, types, lens, meas


def still_state(x):
    """the same head, every clone the identity with zero translation: the depth column of every track is exactly zero"""
    xs = np.array(x, float)
    for c in range((len(xs) - 26) // 7):
        xs[26 + 7 * c: 33 + 7 * c] = [0, 0, 0, 1, 0, 0, 0]
    return xs


STILL_LENS = {10: (7,), 17: (7, 11, 12)}      # type '1': ndof = 2 L - 2 = 12 and 20 (the edges of the register-resident LDL^T templates), 22 (the first even rr of the LDS form)


@functools.lru_cache(maxsize=None)
def still_cases(max_len):
    """(cfg, xs, P1, types, lens, meas): type-'1' tracks of STILL_LENS on the window at rest: N = 2, rho = 0"""
    cfg, x1, P1 = window_state(max_len)
    xs = still_state(x1)
    Ls = STILL_LENS[max_len]
    types, lens, meas = np.full(len(Ls), ord("1"), np.uint8), np.array(Ls, np.int32), np.zeros((len(Ls), max_len, 2), np.float32)
    for f, L in enumerate(Ls):
        meas[f] = _one_track(cfg, xs, max_len, "1", L, STILL_DRAW[max_len][f], extra=1)
    for a in (xs, types, lens, meas):
        a.setflags(write=False)
    return cfg, xs, P1, types, lens, meas


# ---------------------------------------------------------------- the LM branches
LM_CLASSES = ("early-break", "ten-iterations", "reject-then-accept", "rho-negative", "angle-after", "angle-before", "outlier-gated", "zero-depth")


def lm_class_of(tr, accepted=None):
    """the classes of LM_CLASSES a trace (oracle.feature_trace) belongs to — a track can be in several"""
    out = set()
    if tr["invalid"] == "angle-before":
        return {"angle-before"}
    if 0 <= tr["exit_iter"] <= 3:
        out.add("early-break")
    if tr["n_iter"] == 10 and tr["exit_iter"] < 0:
        out.add("ten-iterations")
    st = tr["step"]
    if any((not st[i]) and st[i + 1:].any() for i in range(len(st))):
        out.add("reject-then-accept")
    if tr["invalid"] == "rho-negative":
        out.add("rho-negative")
    if tr["invalid"] == "angle-after":
        out.add("angle-after")
    if tr["valid"] and accepted is not None and not accepted:
        out.add("outlier-gated")
    return out


LM_HAND = LM_CLASSES[:-1]       # built by _lm_track on the recorded window; "zero-depth" lives on the window at rest and comes from still_cases


def _lm_track(cfg, x, max_len, name, k):
    """(type, L, observations) of draw k of the recipe for the class `name` — the recipe only: whether the track reaches the class, and
    whether it meets the conditions, is what the oracle's trace says (LM_DRAW names the first draw that does)"""
    rng = np.random.default_rng([max_len, LM_CLASSES.index(name), k])
    sig = abi.landmark_sigma(cfg)
    ty = "12"[int(rng.integers(0, 2))]
    L = max_len if rng.integers(0, 2) else int(rng.integers(3, max_len + 1))
    near = name in ("ten-iterations", "reject-then-accept", "angle-after")      # a point closer than the window's baseline: the start at rho = 0 is far off
    depth = rng.uniform(0.15, 0.4) if near else rng.uniform(2.0, 8.0)
    pc1 = np.array([rng.uniform(-0.5, 0.5) * depth, rng.uniform(-0.35, 0.35) * depth, depth])
    z = K.project_track(cfg, x, ty, L, pc1)
    nz = sig * rng.standard_normal((L, 2))
    if name == "early-break":                       # noise-free: the cost falls to the rounding of the observations and the loop leaves by its own test
        pass
    elif name == "ten-iterations":
        z = z + nz
    elif name == "reject-then-accept":              # strong noise on a near point: an overshooting step, its cost compared again, a step from there
        z = z + 3 * nz
    elif name == "rho-negative":                    # the parallax mirrored about the bearing of the point at infinity
        zinf = K.project_track(cfg, x, ty, L, pc1 * 1e9)
        z = zinf - (z - zinf) + 1e-3 * nz
    elif name == "angle-after":                     # an outlier on a very near point throws the bearing past 1.57
        z = z + 1e-3 * nz
        z[int(rng.integers(1, L))] += rng.uniform(20, 150) * sig * np.array([1.0, -1.0])
    elif name == "angle-before":                    # psi = atan(fx0) > 1.57 <=> fx0 > 1255.8
        z = z + nz
        z[0, 0] = rng.uniform(1300.0, 5000.0)
    elif name == "outlier-gated":                   # one observation off by 20 .. 150 sigma
        z = z + nz
        z[int(rng.integers(1, L))] += rng.uniform(20, 150) * sig * np.array([1.0, -1.0])
    else:
        raise KeyError(name)
    meas = np.zeros((max_len, 2), np.float32)
    meas[:L] = z
    return ty, L, meas


# window -> the draw per class of LM_HAND that reaches the class and meets the conditions
LM_DRAW = {
    10: (1, 0, 4, 9, 5, 0, 64),
    17: (13, 13, 0, 142, 1, 0, 254),
}


@functools.lru_cache(maxsize=None)
def lm_cases(max_len):
    """(cfg, x, P, names, types, lens, meas): the hand-built tracks of LM_HAND on the recorded window (x1)"""
    cfg, x1, P1 = window_state(max_len)
    types, lens, meas = np.zeros(len(LM_HAND), np.uint8), np.zeros(len(LM_HAND), np.int32), np.zeros((len(LM_HAND), max_len, 2), np.float32)
    for f, name in enumerate(LM_HAND):
        ty, L, m = _lm_track(cfg, x1, max_len, name, LM_DRAW[max_len][f])
        types[f], lens[f], meas[f] = ord(ty), L, m
    for a in (types, lens, meas):
        a.setflags(write=False)
    return cfg, x1, P1, LM_HAND, types, lens, meas


# ---------------------------------------------------------------- measures
def gamma_err(g, t):
    """|gamma - gamma_twin| / gamma_twin; where the twin's residual is exactly zero (gamma_twin = 0), |gamma| itself"""
    gt = float(t["gamma"])
    return abs(float(g) - gt) / gt if gt > 0 else abs(float(g))


def share_err(A, b, t):
    """(eA, eb, outside): max |dA_ij| / sqrt(A_ii A_jj) and max |db_i| / (sqrt(A_ii) |rn|) over the feature's column range — Cauchy-Schwarz bounds
    every entry of A and b by its denominator, so both are errors relative to what the entry could be —, and the largest |entry| of (A, b)
    outside the range (must be exactly 0).  A column of the range whose diagonal entry is exactly zero in the twin (the translation columns at
    rho = 0) belongs to `outside`."""
    At, bt = np.asarray(t["A"], np.longdouble), np.asarray(t["b"], np.longdouble)
    lo, hi = t["cols"]
    dg = np.sqrt(np.diag(At))
    live = np.zeros(len(bt), bool)
    live[lo:hi] = True
    live &= dg > 0
    ix = np.where(live)[0]
    A, b = np.asarray(A, np.longdouble), np.asarray(b, np.longdouble)
    eA = float(np.max(np.abs(A[np.ix_(ix, ix)] - At[np.ix_(ix, ix)]) / np.outer(dg[ix], dg[ix]))) if len(ix) else 0.0
    if t["rn_norm"] > 0:
        eb = float(np.max(np.abs(b[ix] - bt[ix]) / (dg[ix] * t["rn_norm"]))) if len(ix) else 0.0
    else:                                           # the residual is exactly zero: so is every entry of b
        eb = float(np.max(np.abs(b[ix]), initial=0.0))
    dead = ~live
    outside = max(float(np.max(np.abs(A[dead, :]), initial=0.0)), float(np.max(np.abs(A[:, dead]), initial=0.0)), float(np.max(np.abs(b[dead]), initial=0.0)))
    return eA, eb, outside


def backward_err(m, t, sigma):
    """the same three differences on the scales of the operands BEFORE the projection — |d gamma| sigma^2 / |r|^2, |dA_ij| / (|Hx_i| |Hx_j|),
    |db_i| / (|Hx_i| |r|) —: what two correct evaluations in one precision may differ by, whatever the projection cancels"""
    hn, rn = np.asarray(t["hx_norms"], np.longdouble), t["r_norm"]
    lo, hi = t["cols"]
    ix = np.arange(lo, hi)[hn[lo:hi] > 0]
    dA = np.abs(np.asarray(m["A"], np.longdouble) - t["A"])[np.ix_(ix, ix)] / np.outer(hn[ix], hn[ix])
    e = float(np.max(dA, initial=0.0))
    if rn > 0:
        e = max(e, float(abs(np.longdouble(m["gamma"]) - t["gamma"]) * sigma * sigma / (rn * rn)))
        e = max(e, float(np.max(np.abs(np.asarray(m["b"], np.longdouble) - t["b"])[ix] / (hn[ix] * rn), initial=0.0)))
    return e


GAMMA_K, SHARE_K = 400, 1200          # 16 x 22.9 and 16 x 71.0 (both worst ratios on window 32), rounded up


def hf_cond(case, pf):
    """cond of the columns of Hf the projection takes out (the first Lu observations, N columns), in float64, at the triple pf"""
    _, cfg, x, P, ty, L, meas = case
    Hf = abi._feature_rows_as(cfg, x, chr(ty), L, pf, np.float64, with_hx=False, first_exact=True)["Hf"]
    M = 2 * (L if ty == ord("1") else (L + 1) // 2)
    N = 2 if np.sqrt(Hf[:M, 2] @ Hf[:M, 2]) < 1e-4 else 3
    sv = np.linalg.svd(Hf[:M, :N], compute_uv=False)
    return float(sv[0] / sv[-1])


@functools.lru_cache(maxsize=None)
def floors_of(max_len):
    """per case of all_cases(max_len), at the ORACLE's triple: None without a triple, else dict(fg, fs: the error of ONE float64 evaluation of
    the model against the np.longdouble twin in the measures above, cond = hf_cond, bar_g, bar_s: what the device is held to on that case).
    Nothing here is read from the device."""
    out = []
    for case, o in zip(all_cases(max_len), oracle_of(max_len)):
        if not o["valid"]:
            out.append(None)
            continue
        _, cfg, x, P, ty, L, meas = case
        a = (cfg, x, P, chr(ty), L, meas, o["pf"])
        t, m = abi.feature_update_model_as(*a), abi.feature_update_model(*a)
        eA, eb, _ = share_err(m["A"], m["b"], t)
        c = hf_cond(case, o["pf"])
        out.append(dict(fg=gamma_err(m["gamma"], t), fs=max(eA, eb), cond=c, bar_g=min(GAMMA_K * 2.0 ** -52 * c, GAMMA_RTOL_SUITE),
                        bar_s=min(SHARE_K * 2.0 ** -52 * c, SHARE_SUITE)))
    return tuple(out)


def pf_move(pa, pb):
    """scale-free distance of two triples: max |dpf| / (|pf| + 1)"""
    pa, pb = np.asarray(pa, float), np.asarray(pb, float)
    return float(np.max(np.abs(pa - pb) / (np.abs(pb) + 1.0)))


# ---------------------------------------------------------------- conditions
def last_bit_draws(x, meas, L, draws=DRAWS, seed=1):
    """`draws` copies of (x, meas) with every non-zero entry of the state moved by +-1 ulp and every observation by +-1 float32 ulp (the device
    of tests/test_truncation.py::_reference_noise, applied to the inputs of the stage)"""
    rng = np.random.default_rng(seed)
    x, meas = np.asarray(x, float), np.asarray(meas, np.float32)
    for _ in range(draws):
        up = rng.integers(0, 2, x.shape) > 0
        xp = np.where(x != 0, np.nextafter(x, np.where(up, np.inf, -np.inf)), 0.0)
        um = rng.integers(0, 2, meas.shape) > 0
        mp = np.nextafter(meas, np.where(um, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float32)
        mp[L:] = meas[L:]
        yield xp, mp


def trace_key(tr):
    return (tr["valid"], tr["n_iter"], tr["exit_iter"], tr["invalid"], tuple(bool(s) for s in tr["step"]))


def check_conditions(cfg, x, P, ty, L, meas):
    """the conditions a fixed case has to meet; returns (problems [list of str], info dict: trace, diag of the one-feature update, the twin, the
    worst move of the oracle's triple under the last-bit draws)"""
    ty = int(ty)
    tr = O.feature_trace(cfg, x, ty, meas, L)
    _, _, d = O.update(cfg, x, P, [ty], [L], meas[None])
    acc, ndof, gam, pf = int(d["accepted"][0]), int(d["ndof"][0]), float(d["gamma"][0]), d["pfinv"][0]
    bad, move = [], 0.0
    for xp, mp in last_bit_draws(x, meas, L):
        tp = O.feature_trace(cfg, xp, ty, mp, L)
        _, _, dq = O.update(cfg, xp, P, [ty], [L], mp[None])
        if trace_key(tp) != trace_key(tr) or int(dq["ndof"][0]) != ndof or int(dq["accepted"][0]) != acc:
            bad.append("branch trace / ndof / accepted move under last-bit noise")
            break
        if tr["valid"]:
            move = max(move, pf_move(dq["pfinv"][0], pf))
    twin = None
    if tr["valid"] and not bad:
        # the triple itself must not hang on the last bit of the state: the device is held to it at PF_RTOL / PF_ATOL, so the oracle's own
        # triple has to stand 128 times firmer under one ulp on the state alone: the usual factor 16, times 8 for a 3 x 3 solve by another
        # algorithm, which is several ulps of its operands away and not one (a track whose LM path is chaotic does not stand: replaced)
        rng = np.random.default_rng(2)
        xa = np.asarray(x, float)
        for _ in range(16):
            xp = np.where(xa != 0, np.nextafter(xa, np.where(rng.integers(0, 2, xa.shape) > 0, np.inf, -np.inf)), 0.0)
            _, _, dq = O.update(cfg, xp, P, [ty], [L], meas[None])
            if not np.allclose(dq["pfinv"][0], pf, rtol=PF_RTOL / 128, atol=PF_ATOL / 128):
                bad.append("the oracle's triple moves by more than a 128th of the bar under one ulp on the state")
                break
    if tr["valid"]:
        # ... nor on the rounding of the 3 x 3 solve.  A loop that leaves by its own test with a last step below 1e-6 has converged and the solve's
        # error is multiplied by that step; any other exit (ten iterations, a break on a negative depth step) takes its last step at full size,
        # and the reference's rank-revealing QR and the device's L D L^T then differ by c cond(N) 2^-52 of it, N = Hf^T Hf over all L
        # observations, c ~ 30 for a 3 x 3 system: below a 16th of PF_RTOL for cond(N) <= 1e5
        k = tr["exit_iter"]
        if not (k >= 0 and abs(tr["dp2"][k]) < 1e-6):
            Hf = abi._feature_rows_as(cfg, x, chr(ty), L, pf, np.float64, with_hx=False, first_exact=True)["Hf"]
            if not np.linalg.cond(Hf.T @ Hf) <= 1e5:
                bad.append("a full-size last step through an ill-conditioned solve")
        chi = O.chi2_95(ndof)
        if abs(gam - chi) < 1e-6 * chi:
            bad.append("gamma within 1e-6 of its threshold")
        twin = abi.feature_update_model_as(cfg, x, P, chr(ty), L, meas, pf)
        if 0.5e-4 < float(twin["hf2"]) < 2e-4:
            bad.append("|Hf[:, 2]| within a factor 2 of 1e-4")
        r_or = O.feature_model(cfg, x, ty, meas, L)[0]
        if not np.array_equal(r_or, twin["r"].astype(float)):
            bad.append("the twin's float32 residual is not the oracle's")
        if twin["ndof"] != ndof:
            bad.append("ndof: twin %d, oracle %d" % (twin["ndof"], ndof))
    return bad, dict(trace=tr, accepted=acc, ndof=ndof, gamma=gam, pf=pf, twin=twin, pf_move=move)


def in_class(name, info):
    """does the case (info of check_conditions) reach the LM class `name`?  outlier-gated: valid, the loop left by its own test, the gate refused"""
    cl = lm_class_of(info["trace"], info["accepted"])
    if name == "outlier-gated":
        return name in cl and info["trace"]["exit_iter"] >= 0
    return name in cl


def find_draws(max_len, most=400):
    """the tables KIND_DRAW / STILL_DRAW / LM_DRAW for one window: per case the first draw that meets check_conditions (and, for the LM classes,
    reaches its class).  Run by hand when a window or a recipe changes; the result is pasted above."""
    cfg, x1, P1 = window_state(max_len)
    kd, sd, ld = [], [], []
    for ty, L in kinds(max_len):
        kd.append(next(k for k in range(most) if not check_conditions(cfg, x1, P1, ord(ty), L, _one_track(cfg, x1, max_len, ty, L, k))[0]))
    if max_len in STILL_LENS:
        xs = still_state(x1)
        for L in STILL_LENS[max_len]:
            sd.append(next(k for k in range(most) if not check_conditions(cfg, xs, P1, ord("1"), L, _one_track(cfg, xs, max_len, "1", L, k, extra=1))[0]))
    if max_len in LM_WINDOWS:
        for name in LM_HAND:
            for k in range(most):
                ty, L, m = _lm_track(cfg, x1, max_len, name, k)
                bad, info = check_conditions(cfg, x1, P1, ord(ty), L, m)
                if not bad and in_class(name, info):
                    ld.append(k)
                    break
            else:
                raise LookupError((max_len, name))
    return tuple(kd), tuple(sd), tuple(ld)


@functools.lru_cache(maxsize=None)
def all_cases(max_len):
    """every fixed case of one window as (label, cfg, x, P, type code, L, meas [max_len, 2]): the kinds, then the tracks on the window at rest
    and the hand-built LM tracks where the window has them"""
    cfg, x1, P1, types, lens, meas = kind_cases(max_len)
    out = [("kind %s/%d" % (chr(types[f]), lens[f]), cfg, x1, P1, int(types[f]), int(lens[f]), meas[f]) for f in range(len(types))]
    if max_len in STILL_LENS:
        _, xs, _, types, lens, meas = still_cases(max_len)
        out += [("zero-depth 1/%d" % lens[f], cfg, xs, P1, int(types[f]), int(lens[f]), meas[f]) for f in range(len(types))]
    if max_len in LM_WINDOWS:
        _, _, _, names, types, lens, meas = lm_cases(max_len)
        out += [("%s %s/%d" % (names[f], chr(types[f]), lens[f]), cfg, x1, P1, int(types[f]), int(lens[f]), meas[f]) for f in range(len(types))]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def all_infos(max_len):
    """check_conditions of every case of all_cases(max_len), computed once"""
    return tuple(check_conditions(c[1], c[2], c[3], c[4], c[5], c[6]) for c in all_cases(max_len))


@functools.lru_cache(maxsize=None)
def oracle_of(max_len):
    """per case of all_cases(max_len): dict(valid, accepted, ndof, gamma, pf) of the oracle's one-feature update (no last-bit draws)"""
    out = []
    for _, cfg, x, P, ty, L, meas in all_cases(max_len):
        _, _, d = O.update(cfg, x, P, [ty], [L], meas[None])
        tr = O.feature_trace(cfg, x, ty, meas, L)
        out.append(dict(valid=tr["valid"], accepted=int(d["accepted"][0]), ndof=int(d["ndof"][0]), gamma=float(d["gamma"][0]), pf=d["pfinv"][0].copy()))
    return tuple(out)
