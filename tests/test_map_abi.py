"""CPU-side checks of the map-landmark measurement (added within ABI 6): the entry points are exported, declared and named on the ABI-version
line, the structs have the sizes the header states and no padding; NULL handles are refused; abi.map_h — the table of include/rvio_hip.h — is
held to central differences of the predicted image point through the reference's state injection; abi.map_model's zero rows give the update of
the compacted stack; and every case of tests/map_cases.py lies far enough from every decision that device and model cannot disagree on one by
rounding.  No compute is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_cases as M

abi, A = M.abi, M.A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_update_map", "rvio_hip_update_map_dev", "rvio_hip_get_map", "rvio_hip_get_map_rows")
STEP = 1e-6
CALS = M.calibrations()


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
    version_line = [l for l in hdr.splitlines() if l.startswith("#define RVIO_HIP_ABI_VERSION")][0]
    assert "#define RVIO_HIP_ABI_VERSION 6" in version_line and all(s in version_line for s in NEW)
    assert (abi.RVIO_MAP_NORMALISED, abi.RVIO_MAP_PIXELS, abi.RVIO_MAP_MAX_POINTS) == (0, 1, 8)
    assert re.search(r"RVIO_MAP_NORMALISED\s*=\s*0\b", hdr) and re.search(r"RVIO_MAP_PIXELS\s*=\s*1\b", hdr) and "#define RVIO_MAP_MAX_POINTS 8" in hdr
    assert callable(abi.map_h) and callable(abi.map_model)


def _c_struct(hdr, name):
    """(size, offsets) of a struct of doubles and int32s as the header declares it, laid out with natural alignment"""
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), hdr, re.S).group(1)
    off, offs, align = 0, {}, 1
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        ty, rest = decl.split(None, 1)
        w = {"double": 8, "int32_t": 4}[ty]
        align = max(align, w)
        for item in [i.strip() for i in rest.split(",")]:
            mm = re.match(r"(\w+)(?:\[(\d+)\])?$", item)
            off = (off + w - 1) // w * w
            offs[mm.group(1)] = off
            off += w * int(mm.group(2) or 1)
    return (off + align - 1) // align * align, offs


@pytest.mark.parametrize("name,cls,size", [("rvio_map_obs", "rvio_map_obs", 48), ("rvio_map_point", "rvio_map_point", 40), ("rvio_map_diag", "rvio_map_diag", 32)])
def test_struct_sizes_without_padding(name, cls, size):
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    c_size, offs = _c_struct(hdr, name)
    st = getattr(abi, cls)
    assert c_size == size == C.sizeof(st)
    assert sum(C.sizeof(t) for _, t in st._fields_) == size, "padding"
    for f, _ in st._fields_:
        assert getattr(st, f).offset == offs[f], f


def test_null_arguments_are_invalid(lib):
    obs = abi.make_map_obs([((0, 0, 5), (0, 0), 0.01)])
    a = C.c_int(0)
    rec = abi.rvio_map_diag()
    m, d = C.c_int32(0), C.c_int32(0)
    assert lib.rvio_hip_update_map(None, 0, 0, 0, 1, 0, 1, obs) == -1
    assert lib.rvio_hip_update_map_dev(None, 0, 0, 1, 1, obs, C.c_size_t(0), None, C.byref(a), None) == -1
    assert lib.rvio_hip_get_map(None, 0, C.byref(rec), None) == -1
    assert lib.rvio_hip_get_map_rows(None, 0, C.byref(m), C.byref(d), None, None, None) == -1


# ---------------------------------------------------------------- the table against finite differences
def zero_cols(n, age):
    live = set(range(0, 6)) | {24 + 6 * i + c for i in range(n - age, n) for c in range(6)}
    return [c for c in range(24 + 6 * n) if c not in live]


@pytest.mark.parametrize("cal", sorted(CALS))
@pytest.mark.parametrize("n", M.WINDOWS)
def test_jacobian_against_central_differences(n, cal):
    x, P = M.state(n)
    k = CALS[cal]
    T = np.array(k.T_bc[:]).reshape(4, 4)
    assert np.max(np.abs(T[0:3, 0:3] - np.eye(3))) > 0.5 and np.linalg.norm(T[0:3, 3]) > 0.05, "a non-trivial T_bc"
    d = 24 + 6 * n
    for a in M.ages(n):
        for p_w, uv, sg in M.observations(k, x, a, [M.GOOD] * 2, seed=n + a):
            H, h, depth = abi.map_h(k, x, a, p_w)
            assert H.shape == (2, d) and depth >= 0.5
            Hfd = np.zeros_like(H)
            for c in range(d):
                e = np.zeros(d)
                e[c] = STEP
                Hfd[:, c] = (abi.map_h(k, abi.inject_state(x, e), a, p_w)[1] - abi.map_h(k, abi.inject_state(x, -e), a, p_w)[1]) / (2 * STEP)
            worst, top = float(np.max(np.abs(Hfd - H))), float(np.max(np.abs(H)))
            print("n=%d age=%d %s: max|H - FD| = %.3e (bar %.3e, max|H| %.3g)" % (n, a, cal, worst, 1e-6 * top, top))
            assert worst <= 1e-6 * top
            zc = zero_cols(n, a)
            assert not H[:, zc].any() and not Hfd[:, zc].any(), "a column the table lists as 0"
            assert np.abs(H[:, 0:6]).sum() > 0.1 and (a == 0 or np.abs(H[:, 24 + 6 * (n - a): 24 + 6 * n]).sum() > 0.1)


# ---------------------------------------------------------------- zero rows = the compacted stack
@pytest.mark.parametrize("gate_each", [0, 1])
def test_zero_rows_give_the_update_of_the_compacted_stack(gate_each):
    cal, x, P, age, pts = M.gate_case()
    obs = abi.make_map_obs(pts)
    H, r, sg, gamma, status = abi.map_model(cal, x, P, obs, age, abi.RVIO_MAP_NORMALISED, gate_each)
    want = list(M.GATE_STATUS) if gate_each else [0, 0, 0, 0, 2, 0, 0, 0]
    assert list(status) == want
    used = [j for j in range(8) if status[j] == 0]
    for j in range(8):
        rows = slice(2 * j, 2 * j + 2)
        if j in used:
            assert np.abs(H[rows]).sum() > 0.1 and np.all(sg[rows] == M.SIGMA)
        else:
            assert not H[rows].any() and not r[rows].any() and np.all(sg[rows] == 1.0)
    keep = np.array([2 * j + i for j in used for i in (0, 1)])
    x0, P0, g0 = abi.aux_update_model(x, P, H, r, sg)
    x1, P1, g1 = abi.aux_update_model(x, P, H[keep], r[keep], sg[keep])
    import scenarios as S
    dx, dp = S.state_delta(x0, x1), float(np.max(np.abs(P0 - P1)))
    print("gate_each=%d: %d used; zero rows vs compacted: state %.3e (bar %.0e)  P %.3e (bar %.3e)  gamma %.6g vs %.6g" % (gate_each, len(used), dx, A.X_TOL, dp, A.p_bar(P1), g0, g1))
    assert dx <= A.X_TOL and dp <= A.p_bar(P1) and abs(g0 - g1) <= 1e-9 * g1
    assert np.max(np.abs(x0 - x)) > 1e-8


# ---------------------------------------------------------------- the cases keep their distance from every decision
def test_every_case_satisfies_its_own_conditions():
    chi = abi.MAP_CHI2_95_2
    assert abs(chi - A.chi2_95(2)) < 1e-6
    n_cases = 0
    for n, a, k, cal, seed in M.row_cases() + M.row_cases(M.GPU_WINDOWS, M.gpu_ages):
        x, P = M.state(n)
        pts = M.observations(CALS[cal], x, a, [M.GOOD] * k, seed)
        H, r, sg, gamma, status = abi.map_model(CALS[cal], x, P, abi.make_map_obs(pts), a, abi.RVIO_MAP_NORMALISED, 1)
        assert not status.any(), (n, a, k, status)
        for j, (p_w, uv, s) in enumerate(pts):
            assert abi.map_h(CALS[cal], x, a, p_w)[2] >= 0.5 and gamma[j] <= 0.9 * chi
        n_cases += 1
    cal, x, P, age, pts = M.gate_case()
    H, r, sg, gamma, status = abi.map_model(cal, x, P, abi.make_map_obs(pts), age, abi.RVIO_MAP_NORMALISED, 1)
    g0 = abi.map_model(cal, x, P, abi.make_map_obs(pts), age, abi.RVIO_MAP_NORMALISED, 0)[3]
    assert tuple(status) == M.GATE_STATUS
    for j, kind in enumerate(M.GATE_KINDS):
        depth = abi.map_h(cal, x, age, pts[j][0])[2]
        if kind == M.BEHIND:
            assert depth <= -0.5
        else:
            assert depth >= 0.5 and abs(g0[j] - chi) >= 0.1 * chi
            assert (g0[j] > 100) if kind == M.OUTLIER else (g0[j] < 0.9 * chi)
    for name, k in CALS.items():           # the pixel cases: in front of the camera
        for n in (3, 10):
            x, P = M.state(n)
            for p_w, px, s in M.pixel_observations(k, x, n // 2, 8, seed=n):
                assert abi.map_h(k, x, n // 2, p_w)[2] >= 0.5
    print("%d rows cases, the gate case (gammas %s), the pixel cases" % (n_cases, np.array2string(g0, precision=3)))
