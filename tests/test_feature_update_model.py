"""CPU-side checks of the truth the per-feature stage of the update is held to on the device (abi.feature_update_model[_as], the cases of
tests/feature_cases.py): the float64 model against the oracle's gate and information block, the independence of everything the stage hands on
from the nullspace basis, the float64 model's floor against its np.longdouble twin (what the device bars rest on), and the conditions every
fixed case has to meet, with the census of what the cases reach.  No compute is launched here."""
import numpy as np
import pytest

import feature_cases as F
import oracle as O

abi = O.abi
ORACLE_TOL = 1e-11          # the project's bar for a float64 model against the oracle (tests/test_landmark_cov_model.py: ROW_TOL), as a backward error
# Givens against Householder in np.longdouble, as a backward error (F.backward_err): at most M rotations per column against one reflector, M <= 64
# rows, three columns, each step good to an ulp of 2^-63, through S^-1 with cond(S) < 1024 on these cases: 3 * 64 * 1024 * 2^-63 = 2.1e-14
BASIS_TOL = 3 * 64 * 1024 * 2.0 ** -63


def models(case, pf, **kw):
    _, cfg, x, P, ty, L, meas = case
    a = (cfg, x, P, chr(ty), L, meas, pf)
    return abi.feature_update_model_as(*a, **kw), abi.feature_update_model(*a, **kw)


@pytest.mark.parametrize("max_len", F.WINDOWS)
def test_float64_model_against_the_oracle(max_len):
    """gamma, ndof and accepted of O.update's diag per case at the oracle's own triple, and the sum of the accepted shares against the block of
    O.update_local(..., 0, 1) on the table of the window's kinds: the twin is the restatement's U3 .. U5, which tests/test_ref_pins.py pins to
    the reference's sources"""
    cases, infos = F.all_cases(max_len), F.all_infos(max_len)
    worst_g = 0.0
    sig = abi.landmark_sigma(cases[0][1])
    for case, (_, info) in zip(cases, infos):
        if not info["trace"]["valid"]:
            assert info["ndof"] == 0 and info["accepted"] == 0 and info["gamma"] == 0.0, case[0]
            continue
        m = abi.feature_update_model(case[1], case[2], case[3], chr(case[4]), case[5], case[6], info["pf"])
        assert m["ndof"] == info["ndof"] == 2 * m["Lu"] - m["N"], case[0]
        assert (m["gamma"] < O.chi2_95(m["ndof"])) == bool(info["accepted"]), case[0]
        if m["r_norm"] > 0:
            worst_g = max(worst_g, abs(m["gamma"] - info["gamma"]) * sig * sig / m["r_norm"] ** 2)
        else:
            assert info["gamma"] == 0.0 == m["gamma"]
    cfg, x1, P1, types, lens, meas = F.kind_cases(max_len)
    n = max_len - 1
    c6, ld = 6 * n, 6 * n + 1
    blk = O.update_local(cfg, x1, P1, types, lens, meas, 0, 1)
    assert blk[2 * c6 * ld + 5] != 1, "the oracle replaced the sums by its literal sweep"
    Ab = (blk[: c6 * ld] + blk[c6 * ld: 2 * c6 * ld]).reshape(c6, ld)
    _, _, d = O.update(cfg, x1, P1, types, lens, meas)
    A, b, h2, r2 = np.zeros((c6, c6)), np.zeros(c6), np.zeros(c6), 0.0
    for f in range(len(types)):
        if d["accepted"][f]:
            m = abi.feature_update_model(cfg, x1, P1, chr(types[f]), int(lens[f]), meas[f], d["pfinv"][f])
            A, b, h2, r2 = A + m["A"], b + m["b"], h2 + m["hx_norms"] ** 2, r2 + m["r_norm"] ** 2
    assert d["accepted"].sum() == blk[2 * c6 * ld] >= 0.7 * len(types)
    hn = np.sqrt(h2)
    eA = np.max(np.abs(A - Ab[:, :c6]) / np.outer(hn, hn))
    eb = np.max(np.abs(b - Ab[:, c6]) / (hn * np.sqrt(r2)))
    print("max_track_len %d: float64 model vs oracle: gamma %.1e, sum of shares A %.1e b %.1e" % (max_len, worst_g, eA, eb))
    assert worst_g <= ORACLE_TOL and eA <= ORACLE_TOL and eb <= ORACLE_TOL


@pytest.mark.parametrize("max_len", F.WINDOWS)
def test_basis_invariance(max_len):
    """gamma, A and b with Q_f from the reference's Givens sweep equal those from Householder reflectors, to the floor of np.longdouble"""
    worst = 0.0
    for case, (_, info) in zip(F.all_cases(max_len), F.all_infos(max_len)):
        if not info["trace"]["valid"]:
            continue
        h, _ = models(case, info["pf"])
        g, _ = models(case, info["pf"], basis="givens")
        assert h["A"].dtype == np.longdouble and g["N"] == h["N"]
        worst = max(worst, F.backward_err(g, h, np.longdouble(abi.landmark_sigma(case[1]))))
        assert F.share_err(g["A"], g["b"], h)[2] == 0.0, case[0]
    print("max_track_len %d: Givens vs Householder in long double: %.1e (bar %.1e)" % (max_len, worst, BASIS_TOL))
    assert worst <= BASIS_TOL


@pytest.mark.parametrize("max_len", F.WINDOWS)
def test_float64_floor_against_the_twin(max_len):
    """the float64 model's own error against np.longdouble on every fixed case at the oracle's triple, in the measures of the device test, and its
    ratio to 2^-52 cond(Hf): 16 x the worst ratio over the windows is what F.GAMMA_K / F.SHARE_K round up (by less than a factor 2: window 32
    holds both worst ratios), and no bar is looser than what the suite held before"""
    eps = 2.0 ** -52
    fg, fs, rg, rs, cond, cs = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    for case, (_, info), f in zip(F.all_cases(max_len), F.all_infos(max_len), F.floors_of(max_len)):
        if not info["trace"]["valid"]:
            assert f is None
            continue
        assert f["bar_g"] <= F.GAMMA_RTOL_SUITE and f["bar_s"] <= F.SHARE_SUITE, case[0]
        fg, fs, cond, cs = max(fg, f["fg"]), max(fs, f["fs"]), max(cond, f["cond"]), max(cs, info["twin"]["S_cond"])
        rg, rs = max(rg, f["fg"] / (eps * f["cond"])), max(rs, f["fs"] / (eps * f["cond"]))
    print("max_track_len %d: float64 floor gamma %.2e share %.2e; / (2^-52 cond(Hf)): %.1f and %.1f; cond(Hf) <= %.1e, cond(S) <= %.1f" % (max_len, fg, fs, rg, rs, cond, cs))
    assert 16 * rg <= F.GAMMA_K and 16 * rs <= F.SHARE_K
    if max_len == 32:
        assert F.GAMMA_K <= 2 * 16 * rg and F.SHARE_K <= 2 * 16 * rs
    assert cs < 1024.0          # (BASIS_TOL)


@pytest.mark.parametrize("max_len", F.WINDOWS)
def test_conditions_on_the_fixed_cases(max_len):
    """every case: the oracle's branch trace, ndof and accepted unchanged under 16 last-bit draws, gamma away from its threshold, |Hf[:, 2]| away
    from 1e-4, the twin's float32 residual the oracle's; the census: every (type, L) of the window, N = 2 where the window is at rest, and all
    eight LM classes where the window has the hand-built tracks"""
    cases, infos = F.all_cases(max_len), F.all_infos(max_len)
    for case, (bad, _) in zip(cases, infos):
        assert not bad, (case[0], bad)
    nk = len(F.kinds(max_len))
    assert [(chr(c[4]), c[5]) for c in cases[:nk]] == F.kinds(max_len)
    assert {c[5] for c in cases[:nk] if c[4] == ord("1")} == set(range(2, max_len + 1)) and {c[5] for c in cases[:nk] if c[4] == ord("2")} == set(range(3, max_len + 1))
    assert all(i["trace"]["valid"] and i["twin"]["N"] == 3 for _, i in infos[:nk])
    move_kind = max(i["pf_move"] for _, i in infos[:nk])
    census = {}
    for case, (_, info) in zip(cases[nk:], infos[nk:]):
        if case[0].startswith("zero-depth"):
            t = info["twin"]
            assert t["N"] == 2 and t["hf2"] == 0 and info["pf"][2] == 0.0 and info["ndof"] == 2 * case[5] - 2 and info["accepted"] == 1
            census.setdefault("zero-depth", []).append(case[0])
            move_kind = max(move_kind, info["pf_move"])
        for name in F.lm_class_of(info["trace"], info["accepted"]):
            census.setdefault(name, []).append(case[0])
    move_lm = max([i["pf_move"] for c, (_, i) in zip(cases[nk:], infos[nk:]) if not c[0].startswith("zero-depth")], default=0.0)
    print("max_track_len %d: %d kinds, ndof 1 .. %d; the oracle's triple moves by <= %.2e (kinds, zero depth) / %.2e (LM tracks) under last-bit noise"
          % (max_len, nk, max(i["ndof"] for _, i in infos), move_kind, move_lm))
    for name, who in census.items():
        print("   %-20s %s" % (name, ", ".join(who)))
    if max_len in F.LM_WINDOWS:
        _, _, _, names, types, lens, meas = F.lm_cases(max_len)
        for f, name in enumerate(names):
            assert F.in_class(name, infos[nk + len(F.STILL_LENS[max_len]) + f][1]), name
        assert set(census) >= set(F.LM_CLASSES), census
    if max_len in F.STILL_LENS:
        assert {i["ndof"] for c, (_, i) in zip(cases, infos) if c[0].startswith("zero-depth")} == {2 * L - 2 for L in F.STILL_LENS[max_len]}
    # the bar of one form's triple against another's: 16 x the worst of these moves over the windows (window 10's LM tracks), rounded up
    assert 16 * max(move_kind, move_lm) <= F.PF_FORM_BAR
    if max_len == 10:
        assert F.PF_FORM_BAR <= 2 * 16 * move_lm
