"""CPU-side checks of the landmark covariance (csrc/landmark_cov.hip, abi.landmark_cov_model[_as]): the model's raw Jacobians against the
oracle's and against central differences, a Monte-Carlo proof that the formula IS the covariance of the published point (and that two
plausible wrong formulas are not), the float64 model's floor against its extended-precision twin, the C-ABI surface added within ABI 6 and
the launch form.  No compute is launched here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import landmark_cov_cases as K
import oracle as O
from test_aux_plan import static_lds  # noqa: F401  (the fixture that reads the code object's notes)

abi = O.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_set_landmark_cov", "rvio_hip_get_landmark_cov", "rvio_hip_get_landmark_cov_at", "rvio_hip_get_landmark_cov_dev")
FIELDS = ("feat", "n_obs", "status", "reserved", "rho", "rho_sigma", "p_r", "p_w", "cov_r", "cov_w")
ROW_TOL = 1e-11          # the project's bar for a float64 model against the oracle, here relative to the largest entry of the block compared
LIMIT = 163840


@pytest.fixture(scope="module")
def case_b():
    """the stock window of configuration B (10 clones): the tables, and the oracle's own (phi, psi, rho) per feature"""
    cfg, x1, P1, types, lens, meas = K.window_case(11)
    pf = [O.feature_model(cfg, x1, types[f], meas[f], lens[f])[3] for f in range(len(types))]
    return cfg, x1, P1, types, lens, meas, pf


def pick_kinds(types, lens, pf):
    """one feature of every (type, L) of the table whose estimate has rho > 0"""
    seen, out = set(), []
    for f in range(len(types)):
        key = (int(types[f]), int(lens[f]))
        if key not in seen and pf[f][2] > 0:
            seen.add(key)
            out.append(f)
    return out


# ---------------------------------------------------------------- Jacobians
def test_raw_jacobians_against_the_oracle(case_b):
    """Hf, Hx before the nullspace projection at the oracle's own estimate: every row of a type-'1' track, the first 2 ceil(L / 2) rows of a
    type-'2' track (the oracle halves there, Updater.cc:271-275; the rows it returns must agree)"""
    cfg, x1, P1, types, lens, meas, pf = case_b
    feats = pick_kinds(types, lens, pf)
    assert {int(types[f]) for f in feats} == {ord("1"), ord("2")} and {int(lens[f]) for f in feats} >= set(range(2, 12))
    worst = 0.0
    for f in feats:
        _, Hx, Hf, _ = O.feature_model(cfg, x1, types[f], meas[f], lens[f], pf[f])
        rows = Hx.shape[0]
        assert rows == (2 * ((lens[f] + 1) // 2) if types[f] == ord("2") else 2 * lens[f])
        m = abi.landmark_cov_model(cfg, x1, P1, chr(types[f]), int(lens[f]), meas[f], pf[f])
        assert m["Hx"].shape == (2 * lens[f], Hx.shape[1]) and m["Hf"].shape == (2 * lens[f], 3)
        ex = np.abs(m["Hx"][:rows] - Hx).max() / max(1.0, np.abs(Hx).max())
        ef = np.abs(m["Hf"][:rows] - Hf).max() / max(1.0, np.abs(Hf).max())
        worst = max(worst, ex, ef)
        assert ex <= ROW_TOL and ef <= ROW_TOL, (f, ex, ef)
        lo, hi = m["span"]
        assert (lo, hi) == ((24 + 6 * (10 - (lens[f] - 1)), 84) if types[f] == ord("1") else (24, 24 + 6 * (lens[f] - 1)))
        keep = np.zeros(Hx.shape[1], bool)
        keep[lo - 24: hi - 24] = True
        assert not m["Hx"][:, ~keep].any() and not m["Jx"][:, ~keep].any()
    print("model vs oracle, raw Hf / Hx rows: worst %.2e" % worst)


def test_jacobians_against_central_differences(case_b):
    """what the oracle does not return — the later rows of a type-'2' track — and Jtheta, Jx and the (qG, pG) columns of M_w, against central
    differences through abi.inject_state of an independent projection (landmark_cov_cases.project_track) and of the point itself"""
    cfg, x1, P1, types, lens, meas, pf = case_b
    n, d, h = 10, 84, 1e-6
    for f in (next(f for f in range(len(types)) if types[f] == ord("2") and pf[f][2] > 0), next(f for f in range(len(types)) if types[f] == ord("1") and lens[f] == 6)):
        ty, L = chr(types[f]), int(lens[f])
        m = abi.landmark_cov_model(cfg, x1, P1, ty, L, meas[f], pf[f])
        Hx_fd, Jx_fd, Jw_fd = np.zeros((2 * L, d)), np.zeros((3, d)), np.zeros((3, d))
        for k in range(d):
            dx = np.zeros(d)
            dx[k] = h
            xp, xm = abi.inject_state(x1, dx), abi.inject_state(x1, -dx)
            Hx_fd[:, k] = (K.residuals(cfg, xm, ty, L, meas[f], pf[f]) - K.residuals(cfg, xp, ty, L, meas[f], pf[f])) / (2 * h)      # r = z - h: dr = -H dx
            (rp, wp), (rm, wm) = K.point_of(cfg, xp, ty, L, pf[f]), K.point_of(cfg, xm, ty, L, pf[f])
            Jx_fd[:, k], Jw_fd[:, k] = (rp - rm) / (2 * h), (wp - wm) / (2 * h)
        Hf_fd, Jt_fd = np.zeros((2 * L, 3)), np.zeros((3, 3))
        for k in range(3):
            dp = np.zeros(3)
            dp[k] = h
            Hf_fd[:, k] = (K.residuals(cfg, x1, ty, L, meas[f], pf[f] - dp) - K.residuals(cfg, x1, ty, L, meas[f], pf[f] + dp)) / (2 * h)
            Jt_fd[:, k] = (K.point_of(cfg, x1, ty, L, pf[f] + dp)[0] - K.point_of(cfg, x1, ty, L, pf[f] - dp)[0]) / (2 * h)
        assert not Hx_fd[:, :24].any()                       # the observations depend on the track's clones only
        RG = abi.quat_to_rot(x1[0:4])
        Jw = np.hstack([m["M_w"][:, :24], RG.T @ m["Jx"]])   # d p_w / d x at fixed theta: the head columns of M_w, R_G^T Jx over the clones
        for name, a, b in (("Hx", m["Hx"], Hx_fd[:, 24:]), ("Hf", m["Hf"], Hf_fd), ("Jtheta", m["Jtheta"], Jt_fd), ("Jx", m["Jx"], Jx_fd[:, 24:]), ("Jw", Jw, Jw_fd)):
            e = np.abs(a - b).max() / np.abs(b).max()
            assert e <= 1e-7, (f, name, e)                   # central differences at h = 1e-6: h^2 truncation + eps / h rounding
        assert not Jx_fd[:, :24].any() and np.abs(Jw_fd[:, :6]).max() > 0.5


# ---------------------------------------------------------------- the formula is the covariance
def sample_cov(cfg, x1, Lp, ty, L, z0, pf0, s, sig, K_, rng):
    """second moments (about the linearisation point, / s^2) of p_r, p_w and rho over K_ draws: x through abi.inject_state with dx = s Lp g,
    the observations z0 + s sigma g', theta re-solved by Gauss-Newton per draw"""
    r0, w0 = K.point_of(cfg, x1, ty, L, pf0)
    Sr, Sw, St = np.zeros((3, 3)), np.zeros((3, 3)), 0.0
    d = Lp.shape[0]
    for _ in range(K_):
        xs = abi.inject_state(x1, s * (Lp @ rng.standard_normal(d))) if Lp.any() else x1
        zs = z0 + s * sig * rng.standard_normal(z0.shape)
        pf = K.solve_theta(cfg, xs, ty, L, zs, pf0, iters=4)
        pr, pw = K.point_of(cfg, xs, ty, L, pf)
        Sr += np.outer(pr - r0, pr - r0)
        Sw += np.outer(pw - w0, pw - w0)
        St += (pf[2] - pf0[2]) ** 2
    return Sr / (K_ * s * s), Sw / (K_ * s * s), St / (K_ * s * s)


def test_monte_carlo_the_formula_is_the_covariance():
    """Fixture B of tests/golden/full_load_inputs.npz, a type-'2' track (feature 12, L = 11) and a type-'1' track (feature 9, L = 10): of the
    fixture's tracks the ones on which the state term weighs most against the pixel noise at its true size (sigma_im = 1 px in normalised
    units: the noise term is 70 .. 95 % of the standard deviation of most points).  K draws per run, the bar 5 sqrt(2 / K) on every
    correlation-normalised entry (a Gaussian sample covariance's own scatter); s = 0.02 so that second-order terms vanish (state sd <= 15 cm
    -> 3 mm); sigma = sigma_im unscaled in the formula and s sigma in the draws.  Run 1: x ~ N(x1, s^2 P), noisy observations — the formula
    holds, and both wrong formulas (Jx P Jx^T + noise, without the triangulation's own dependence on the clones; the noise term alone)
    miss the bar: they are off by 0.67 / 0.65 (feature 12: K = 500, bar 0.224) and 0.30 / 0.30 (feature 9: K = 2000, bar 0.158) in that
    metric.  Run 2, K = 500: P = 0 — the sigma^2 N^-1 term at its true size, and the state term alone is not it."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import golden_io as M
    cfg, x1, P1, types, lens, meas = M.load_full_load_case(np.load(os.path.join(ROOT, "tests", "golden", "full_load_inputs.npz")), "B")
    pf = {f: O.feature_model(cfg, x1, types[f], meas[f], lens[f])[3] for f in (12, 9)}
    s = 0.02
    sig = abi.landmark_sigma(cfg)
    assert sig == float(max(np.float32(cfg.sigma_px), np.float32(cfg.sigma_py)))          # already in normalised units: not divided by fx
    w, V = np.linalg.eigh(P1)
    Lp = V * np.sqrt(np.maximum(w, 0.0))
    rng = np.random.default_rng(7)
    assert (chr(types[12]), lens[12], chr(types[9]), lens[9]) == ("2", 11, "1", 10)
    for f, Kn in ((12, 500), (9, 2000)):
        bar = 5 * np.sqrt(2.0 / Kn)
        ty, L = chr(types[f]), int(lens[f])
        pf0 = K.solve_theta(cfg, x1, ty, L, meas[f], pf[f])
        e = np.array([np.cos(pf0[0]) * np.sin(pf0[1]), np.sin(pf0[0]), np.cos(pf0[0]) * np.cos(pf0[1])])
        z0 = K.project_track(cfg, x1, ty, L, e / pf0[2])                    # residual-free observations of the linearisation point
        m = abi.landmark_cov_model(cfg, x1, P1, ty, L, z0, pf0)
        noise_r = sig * sig * (m["Jtheta"] @ np.linalg.solve(m["N"], m["Jtheta"].T))
        wrong_a = noise_r + m["Jx"] @ P1[24:, 24:] @ m["Jx"].T
        Sr, Sw, St = sample_cov(cfg, x1, Lp, ty, L, z0, pf0, s, sig, Kn, rng)
        er, ew, et = K.cov_err(Sr, m["cov_r"]), K.cov_err(Sw, m["cov_w"]), abs(St / m["rho_sigma"] ** 2 - 1)
        ea, eb = K.cov_err(wrong_a, Sr), K.cov_err(noise_r, Sr)
        print("type %s L %d: sample / formula variances r %s w %s, e_r %.3f e_w %.3f rho %.3f (bar %.3f); without Jth A Hx %.2f, noise only %.2f; state / noise sd %.1f"
              % (ty, L, np.diag(Sr) / np.diag(m["cov_r"]), np.diag(Sw) / np.diag(m["cov_w"]), er, ew, et, bar, ea, eb, np.sqrt(np.trace(m["cov_r"] - noise_r) / np.trace(noise_r))))
        assert er <= bar and ew <= bar and et <= bar
        assert ea > bar and eb > bar, "a wrong formula passes: the test cannot fail"
        # noise only
        m0 = abi.landmark_cov_model(cfg, x1, np.zeros_like(P1), ty, L, z0, pf0)
        assert K.cov_err(m0["cov_r"], noise_r) <= 1e-12
        bar0 = 5 * np.sqrt(2.0 / 500)
        Sr0, Sw0, St0 = sample_cov(cfg, x1, np.zeros_like(P1), ty, L, z0, pf0, s, sig, 500, rng)
        e0 = max(K.cov_err(Sr0, m0["cov_r"]), K.cov_err(Sw0, m0["cov_w"]), abs(St0 / m0["rho_sigma"] ** 2 - 1))
        print("   P = 0: e %.3f, noise sd of p_r %s m" % (e0, np.sqrt(np.diag(m0["cov_r"]))))
        assert e0 <= bar0
        assert K.cov_err(m["cov_r"] - noise_r, Sr0) > bar0         # ... and the state term alone is not it


@pytest.mark.parametrize("max_len", K.WINDOWS)
def test_float64_floor_against_the_twin(max_len):
    """the float64 model's own error against np.longdouble on the device tests' cases: below 1e-12, so those cases take the 1e-11 bar"""
    cfg, x1, P1, types, lens, meas = K.window_case(max_len)
    _, _, d = O.update(cfg, x1, P1, types, lens, meas)
    floor, cond, cnt = 0.0, 0.0, 0
    for f in range(len(types)):
        if not d["accepted"][f] or not d["pfinv"][f][2] > 0:
            continue
        a = (cfg, x1, P1, chr(types[f]), int(lens[f]), meas[f], d["pfinv"][f])
        t, m = abi.landmark_cov_model_as(*a), abi.landmark_cov_model(*a)
        assert t["cov_r"].dtype == np.longdouble and m["cov_r"].dtype == np.float64 and m["status"] == 0
        assert np.array_equal(m["cov_r"], m["cov_r"].T) and np.array_equal(m["cov_w"], m["cov_w"].T)
        floor = max(floor, K.cov_err(m["cov_r"], t["cov_r"]), K.cov_err(m["cov_w"], t["cov_w"]))
        cond = max(cond, float(np.linalg.cond(m["N"])))
        cnt += 1
    print("max_track_len %d: %d cloud members, float64 floor %.2e, cond(N) <= %.1e" % (max_len, cnt, floor, cond))
    assert cnt >= 6 and floor < K.FLOOR_BAR


def test_status_case_is_singular_in_float64():
    """the device test's hand-built case: the newest clone the identity with zero translation — the depth column of an L = 2 type-'1' track is
    exactly zero, N_22 = 0, the third pivot is not positive: status 1, NaN covariances, finite points"""
    cfg, x1, P1, types, lens, meas = K.window_case(10)
    _, _, d = O.update(cfg, x1, P1, types, lens, meas)
    xs = x1.copy()
    xs[26 + 7 * 8: 26 + 7 * 9] = [0, 0, 0, 1, 0, 0, 0]
    short = [f for f in range(len(types)) if types[f] == ord("1") and lens[f] == 2 and d["accepted"][f] and d["pfinv"][f][2] > 0]
    assert short
    for f in short:
        m = abi.landmark_cov_model(cfg, xs, P1, "1", 2, meas[f], d["pfinv"][f])
        assert m["status"] == abi.LANDMARK_COV_SINGULAR and m["N"][2, 2] == 0.0 and not m["Hf"][:, 2].any()
        assert np.isnan(m["cov_r"]).all() and np.isnan(m["cov_w"]).all() and np.isnan(m["rho_sigma"]) and np.isfinite(m["p_r"]).all() and np.isfinite(m["p_w"]).all()
        assert abi.landmark_cov_model(cfg, x1, P1, "1", 2, meas[f], d["pfinv"][f])["status"] == 0


# ---------------------------------------------------------------- the C-ABI surface
@pytest.fixture(scope="module")
def lib():
    from rvio_amd import build, hip
    build.build()
    return hip.load()


def test_symbols_exported_and_declared_within_abi_6(lib):
    from rvio_amd import hip
    assert abi.ABI_VERSION == 6 and lib.rvio_hip_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    declared = set(re.findall(r"\b(rvio_(?:hip_)?[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in hip.SYMBOLS and hasattr(lib, s), s
    for phrase in ("NOT the cloud's\n * p_world", "posterior-refined landmark", "mixed\n * p_world", "Cov(dx+, dx-) = (I - K H) P-", "between landmarks", "a ring of clouds",
                   "time stamps in the record", "uncertain map points"):
        assert phrase in hdr, phrase


def test_record_layout_matches_a_cxx_compiler_and_the_header_text(tmp_path):
    assert C.sizeof(abi.rvio_landmark_cov) == 224 == abi.LANDMARK_COV_DTYPE.itemsize
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "hostemu", "landmark_cov_layout.cpp"), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[0] == 224
    assert got[1:] == [getattr(abi.rvio_landmark_cov, f).offset for f in FIELDS]
    assert got[1:] == [abi.LANDMARK_COV_DTYPE.fields[f][1] for f in FIELDS]
    assert got[1:] == [0, 4, 8, 12, 16, 24, 32, 56, 80, 152]          # no padding: 4 * 4 + 8 * (2 + 3 + 3 + 9 + 9) = 224
    # the members in the header's order
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    body = re.search(r"typedef struct rvio_landmark_cov \{(.*?)\} rvio_landmark_cov;", hdr, re.S).group(1)
    assert tuple(re.findall(r"(?:int32_t|double)\s+([a-z_]+)(?:\[\d+\])?;", body)) == FIELDS


def test_null_handle_is_invalid(lib):
    n, fr, rec = C.c_int32(0), C.c_int32(0), abi.rvio_landmark_cov()
    assert lib.rvio_hip_set_landmark_cov(None, 1) == -1
    assert lib.rvio_hip_get_landmark_cov(None, C.byref(n), C.byref(fr), C.byref(rec)) == -1
    assert lib.rvio_hip_get_landmark_cov_at(None, 0, C.byref(n), C.byref(fr), C.byref(rec)) == -1
    assert lib.rvio_hip_get_landmark_cov_dev(None, C.byref(rec), C.c_size_t(1), C.byref(n)) == -1
    us = C.c_float(0)
    assert lib.rvio_hip_debug_time_kernel(None, 15, 1, C.byref(us)) == -1


# ---------------------------------------------------------------- the launch form
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("landmark_cov_plan") / "landmark_cov_plan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-variable",
                           os.path.join(ROOT, "tests", "hostemu", "landmark_cov_plan_emu.cpp"), "-o", so])
    L = C.CDLL(so)
    L.lcp_kernel_name.restype = C.c_char_p
    L.lcp_lds_doubles.restype = C.c_long
    L.lcp_pivot_eps.restype = C.c_double
    return L


@pytest.mark.parametrize("batch", [1, 8, 128])
def test_launch_form_over_every_window(emu, batch):
    """one workgroup of four waves per (instance, hand-over slot), no dynamic LDS, at every accepted max_track_len; every non-zero column, every
    observation and every entry has its thread, and the LDS the kernel declares holds the longest track"""
    assert emu.lcp_threads() == 256 and emu.lcp_words() * 8 == C.sizeof(abi.rvio_landmark_cov) and emu.lcp_rows() == 7 and emu.lcp_ents() == 19
    assert emu.lcp_groups() * emu.lcp_ents() <= emu.lcp_threads() and emu.lcp_pivot_eps() == abi.LANDMARK_COV_PIVOT_EPS
    for max_len in range(3, 33):
        n = max_len - 1
        for nf in (2, 200, 4096):
            fu = (nf + 1) // 2
            out = (C.c_long * 6)()
            emu.lcp_launch(batch, fu, out)
            assert list(out) == [fu, 1, batch, 256, 0, emu.lcp_kernel_id()], (max_len, nf)
        assert 6 + 6 * n <= emu.lcp_nz() <= emu.lcp_threads() and max_len <= emu.lcp_lmax() <= 64
    nmax, lmax = emu.lcp_nmax(), emu.lcp_lmax()
    assert emu.lcp_lds_doubles() == nmax * 12 + lmax * 15 + lmax * 24 + 2 * 7 * emu.lcp_nz() + 2 * emu.lcp_groups() * 19 + 96 + emu.lcp_words()
    assert 8 * emu.lcp_lds_doubles() <= LIMIT


@pytest.mark.parametrize("batch", [1, 8, 128])
def test_static_lds_within_a_cu(emu, static_lds, batch):  # noqa: F811
    name = "landmark_cov_kernel"
    names = [emu.lcp_kernel_name(k).decode() for k in range(emu.lcp_num_kernels())]
    assert name in names and name in static_lds and len(set(names)) == len(names) and names[emu.lcp_kernel_id()] == name
    st, counted = static_lds[name], 8 * emu.lcp_lds_doubles()
    print("batch %d: static LDS of %s = %d B (the plan counts %d B), dynamic 0" % (batch, name, st, counted))
    assert counted <= st <= counted + 256 and st <= LIMIT
    statics = (C.c_size_t * len(names))(*[static_lds[nm] for nm in names])
    attr = C.c_long(-1)
    for max_len in (3, 11, 32):
        assert emu.lcp_plan(max_len, 60, batch, statics, emu.lcp_kernel_id(), C.byref(attr)) == 0 and attr.value == 0
    statics[emu.lcp_kernel_id()] = LIMIT + 8
    assert emu.lcp_plan(11, 200, batch, statics, emu.lcp_kernel_id(), C.byref(attr)) == 1
