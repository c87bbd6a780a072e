"""The launch geometry of every accepted configuration, on the CPU.

rvio_hip_create / rvio_hip_create_batch accept max_track_len 3..32, n_features 2..4096 and any batch size; r-vio_amd/csrc/launch_plan.h derives
from them every dynamic-LDS size, the kernel variants and what moves from LDS to global memory, and create_impl applies exactly that text.
tests/hostemu/plan_emu.cpp compiles the same header with g++; this file sweeps EVERY window x EVERY feature count x batch in {1, 8, 128} and
checks, for every kernel that is given a dynamic-LDS limit, that dynamic + static fits the 163 840 B of a gfx950 CU — or that the plan refuses
the configuration with a message.  The forms of an update (update_forms(): which kernels it launches at clone count n) are swept the same way
for every n of every window: roles only where the Joseph launch has them, every launch's dynamic LDS inside its kernel's limit, every threshold
pinned on both sides.  The static part is the compiler's decision: it is read from the BUILT library (the .hip_fatbin section ->
the gfx950 code object -> the kernel descriptors' notes), not from a table — the library must have been built (`__graft_entry__.build()`).

What this would have caught (and the arithmetic of the commit before it, kept here as `parent_book_lds`): book-keeping's LDS was budgeted
against 150 KB without ransac_book_kernel's 15 600 B of static LDS.  At n_features = 1024: 151 568 + 15 600 = 167 168 B; at 2851 (and every
larger count, batch handles included): 148 272 + 15 600 = 163 872 B — both beyond a CU, so such a handle failed with a HIP error.
"""
import ctypes as C
import os
import re
import subprocess

import pytest

from code_object import read_static_lds

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostemu", "plan_emu.cpp")
HDR = os.path.join(ROOT, "r-vio_amd", "csrc", "launch_plan.h")
EMU = os.path.join(HERE, "hostemu", "libplan_emu.so")
LIMIT = 163840
BATCHES = (1, 8, 128)


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(EMU) or os.path.getmtime(EMU) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-variable", SRC, "-o", EMU])
    L = C.CDLL(EMU)
    L.lp_kernel_name.restype = C.c_char_p
    for f in ("lp_lds_limit", "lp_sweep", "lp_diag_end", "lp_block_doubles", "lp_book_lds_bytes"):
        getattr(L, f).restype = C.c_long
    return L


@pytest.fixture(scope="module")
def static_lds():
    """{kernel name as c++filt prints it, without return type and arguments: static LDS in bytes} of the built library's gfx950 code object"""
    return read_static_lds()


@pytest.fixture(scope="module")
def statics(emu, static_lds):
    n = emu.lp_num_kernels()
    arr = (C.c_size_t * n)()
    for k in range(n):
        name = emu.lp_kernel_name(k).decode()
        assert name in static_lds, "kernel %s of launch_plan.h is not in the built library" % name
        arr[k] = static_lds[name]
    return arr


def evaluate(emu, statics, ml, F, batch):
    n = emu.lp_num_kernels()
    attr, info, why = (C.c_size_t * n)(), (C.c_long * 18)(), C.create_string_buffer(256)
    rc = emu.lp_eval(ml, F, batch, statics, attr, info, why)
    keys = ("book_waves", "book_lds", "book_fused", "tm_global", "lit_state_global", "solve5_variant", "solve7_variant", "solve9_nt", "n_ic", "feat_threads",
            "feat_lds", "fprop_lds", "trunc_lds", "fuse_ok", "jb_lds", "gram_batch_lds", "chol_queue", "lit_ok")
    d = dict(zip(keys, info))
    d.update(rc=rc, why=why.value.decode(), attr={emu.lp_kernel_name(k).decode(): int(attr[k]) for k in range(n)})
    return d


def parent_book_lds(F, batch):
    """book_lds as the commit before this test computed it (rvio_hip.hip: 150 KB budget, no static part)"""
    r8 = (20 * F + 7) & ~7
    waves = 4
    if batch == 1:
        for nwv in (16, 8):
            if r8 + nwv * F * 8 + 16 <= 150 * 1024:
                waves = nwv
                break
    return r8 + waves * F * 8 + 16, waves


def test_constants_match_the_header(emu):
    assert emu.lp_lds_limit() == LIMIT
    assert emu.lp_max_len() == 32 and emu.lp_max_features() == 4096
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    assert "2..4096" in hdr.replace(" ", ""), "include/rvio_hip.h must state the supported n_features range"


@pytest.mark.parametrize("batch", BATCHES)
def test_every_configuration_fits_a_cu_or_is_refused(emu, statics, batch):
    n = emu.lp_num_kernels()
    worst, cfgs, bad, uns = (C.c_size_t * n)(), (C.c_int * (2 * n))(), (C.c_int * 3)(), C.c_long(0)
    nbad = emu.lp_sweep(3, 32, 2, 4096, batch, statics, worst, cfgs, bad, C.byref(uns))
    for k in range(n):
        print("batch %3d  %-30s static %6d  worst static + dynamic %6d at max_track_len %2d, n_features %4d"
              % (batch, emu.lp_kernel_name(k).decode(), statics[k], worst[k], cfgs[2 * k], cfgs[2 * k + 1]))
    assert nbad == 0, "%d (configuration, kernel) pairs over %d B; first: %s at max_track_len %d, n_features %d" % (
        nbad, LIMIT, emu.lp_kernel_name(bad[0]).decode(), bad[1], bad[2])
    # what is refused is known and says why: nothing for one instance; for a batch handle nothing either (every window 3..32 has a solve:
    # solve6 at 6n <= 126, the register-tableau kernel at 132 <= 6n <= 186)
    assert uns.value == 0, "%d configurations refused at batch %d" % (uns.value, batch)
    # the sweep saw the large kernels at all (a table of zeros would pass the assertion above)
    tot = {emu.lp_kernel_name(k).decode(): int(worst[k]) for k in range(n)}
    assert tot["bookkeep_b_kernel"] > 140 * 1024 and tot["feat_build_kernel<16>"] > 100 * 1024
    if batch == 1:
        assert tot["ransac_book_kernel"] > 150 * 1024 and tot["solve9_small_kernel"] > 150 * 1024 and tot["feat_prop_kernel"] > 100 * 1024


def test_the_parents_book_keeping_budget_did_not_fit(static_lds):
    """the defect this file was written for, evaluated on the old formula: it must be over the limit, and the new plan (below) must not be"""
    st = static_lds["ransac_book_kernel"]
    assert st >= 15000, st        # (15 600 B when this was written)
    dyn, waves = parent_book_lds(1024, 1)
    assert (dyn, waves) == (151568, 16) and dyn + st > LIMIT
    dyn, waves = parent_book_lds(2851, 1)
    assert (dyn, waves) == (148272, 4) and dyn + st > LIMIT      # (20 F rounded up to 8 bytes: 57 024, not 57 020)
    assert parent_book_lds(2851, 128)[0] + st > LIMIT
    if st == 15600:
        assert parent_book_lds(1024, 1)[0] + st == 167168 and parent_book_lds(2851, 1)[0] + st == 163872
        over = [F for F in range(2, 4097) if parent_book_lds(F, 1)[0] + st > LIMIT]
        assert over == list(range(1002, 1038)) + list(range(1765, 1829)) + list(range(2851, 4097))


@pytest.mark.parametrize("batch", BATCHES)
def test_book_keeping_plan(emu, statics, static_lds, batch):
    """fewer waves first, then the unfused pair (ransac_book_a_kernel + bookkeep_b_kernel: RANSAC needs 256 threads, the refill half any number of waves)"""
    st_f, st_b = static_lds["ransac_book_kernel"], static_lds["bookkeep_b_kernel"]
    seen = set()
    for F in range(2, 4097):
        p = evaluate(emu, statics, 11, F, batch)
        assert p["rc"] == 0, (F, p["why"])
        w = p["book_waves"]
        assert p["book_lds"] == emu.lp_book_lds_bytes(F, w) == p["attr"]["bookkeep_b_kernel"]
        assert w in ((16, 8, 4, 2, 1) if batch == 1 else (4, 2, 1))
        if p["book_fused"]:
            assert w >= 4 and p["attr"]["ransac_book_kernel"] == p["book_lds"] and p["book_lds"] + max(st_f, st_b) <= LIMIT
        else:
            assert p["attr"]["ransac_book_kernel"] == 0 and p["book_lds"] + st_b <= LIMIT
            # not given up early: the fused launch does not fit with four waves
            assert emu.lp_book_lds_bytes(F, 4) + st_f > LIMIT
        if F <= 2048:
            assert p["book_fused"], F          # the one-launch form up to 28 % above cfg E
        if batch == 1 and w < 16:
            assert emu.lp_book_lds_bytes(F, 2 * w) + (max(st_f, st_b) if p["book_fused"] and 2 * w >= 4 else st_b) > LIMIT, F    # as many waves as fit
        seen.add((w, p["book_fused"]))
    assert seen == ({(16, 1), (8, 1), (4, 1), (4, 0), (2, 0)} if batch == 1 else {(4, 1), (4, 0), (2, 0)})
    # the configurations the suite has always run keep their geometry
    if batch == 1:
        for F, w in ((100, 16), (200, 16), (400, 16), (800, 16), (1600, 8)):
            assert evaluate(emu, statics, 11, F, 1)["book_waves"] == w


def test_thresholds_of_the_window(emu, statics):
    """the host's choices by 6n, pinned on both sides of every threshold (the GPU suite runs each of these windows: tests/test_gpu_windows.py)"""
    P = {ml: evaluate(emu, statics, ml, 200, 1) for ml in range(3, 33)}
    B = {ml: evaluate(emu, statics, ml, 200, 128) for ml in range(3, 33)}
    for ml in range(3, 33):
        c6 = 6 * (ml - 1)
        p, b = P[ml], B[ml]
        assert p["solve9_nt"] == (4 if c6 <= 64 else 6 if c6 <= 96 else 8 if c6 <= 128 else 12) and p["solve5_variant"] == (1 if c6 <= 60 else 2 if c6 <= 96 else 3 if c6 <= 126 else 0)
        assert p["solve7_variant"] == 0 and p["n_ic"] == (1 if 96 < c6 <= 192 else 2)
        assert p["feat_threads"] == (128 if c6 + 1 <= 128 else 256)
        assert p["fuse_ok"] == 1 and p["fprop_lds"] >= max(p["feat_lds"], 86432)
        assert b["solve9_nt"] == 0 and b["solve7_variant"] == (0 if c6 <= 126 else 4) and b["tm_global"] == 1 and b["lit_state_global"] == 1
        assert (b["jb_lds"] > 0) == (c6 <= 60) and (b["gram_batch_lds"] > 0) == (b["gram_batch_lds"] <= 65536 and b["gram_batch_lds"] > 0)
        assert (p["attr"]["solve9_small_kernel"] > 0) == (c6 <= 64)
    # T and the literal sweep's state move to global memory at long windows only, and the switch is inside the accepted range
    assert [ml for ml in range(3, 33) if P[ml]["tm_global"]] == list(range(min(ml for ml in P if P[ml]["tm_global"]), 33))
    assert not P[21]["tm_global"] and P[31]["tm_global"]
    assert [ml for ml in range(3, 33) if P[ml]["lit_state_global"]] == list(range(min(ml for ml in P if P[ml]["lit_state_global"]), 33))
    assert not P[11]["lit_state_global"] and P[31]["lit_state_global"]


def test_rejected_configurations_say_why(emu, statics):
    for F in (4097, 4098, 100000):
        p = evaluate(emu, statics, 11, F, 1)
        assert p["rc"] == 1 and "4096" in p["why"]
    for ml, F, batch in ((2, 100, 1), (33, 100, 1), (11, 1, 1), (11, 100, 0)):
        assert evaluate(emu, statics, ml, F, batch)["rc"] == 1


def test_a_fatter_kernel_is_refused_not_launched(emu, static_lds):
    """static LDS is the compiler's: if a later build's kernels grow, the plan must fall back or refuse — never ask for more than a CU has"""
    n = emu.lp_num_kernels()
    names = [emu.lp_kernel_name(k).decode() for k in range(n)]
    fat = (C.c_size_t * n)(*[static_lds[nm] + 8192 for nm in names])
    worst, cfgs, bad, uns = (C.c_size_t * n)(), (C.c_int * (2 * n))(), (C.c_int * 3)(), C.c_long(0)
    assert emu.lp_sweep(3, 32, 2, 4096, 1, fat, worst, cfgs, bad, C.byref(uns)) == 0
    assert uns.value > 0                                   # (solve9_small_kernel's 160 328 B no longer fit: short windows are refused by name)
    p = evaluate(emu, fat, 8, 200, 1)
    assert p["rc"] == 1 and "LDS" in p["why"]


def test_diagnostics_stay_inside_the_block(emu):
    """lit_scan_gram's row norms, and the instrumented build's phase stamps, live in the unused second part of the [A|b] block (2 ldh^2 doubles)"""
    for ml in range(3, 33):
        ldh = 6 * (ml - 1) + 1
        assert emu.lp_block_doubles(ml) == 2 * ldh * ldh
        for stamps in (0, 1):
            end = emu.lp_diag_end(ml, stamps)
            assert ldh * ldh < end <= 2 * ldh * ldh, (ml, stamps, end)
        # (the stamps at ldh^2 + 200..204 have no room at max_track_len = 3 — 369..373 of 338 doubles — and are not written there)
        assert (emu.lp_diag_end(ml, 1) == ldh * ldh + 205) == (ldh * ldh >= 205)
    src = open(os.path.join(ROOT, "r-vio_amd", "csrc", "literal.h")).read()
    m = re.search(r"#ifdef RVIO_DBG_CLOCKS\n#define LIT_STAMP\(k\)[^\n]*lit_stamp_fits[^\n]*\n#else\n#define LIT_STAMP\(k\) do \{ \} while \(0\)\n#endif", src)
    assert m, "LIT_STAMP must be empty in the shipping build and bounded in the instrumented one"
    assert len(re.findall(r"#define LIT_STAMP", src)) == 2


# ---------------------------------------------------------------- update_forms(): the kernels of ONE update, by clone count
CHOL = ("none", "role", "queue")
GRAM = ("reduce", "batch4", "batch6")
TPROD = ("none", "gemm", "gemm_lds")
SOLVE = ("none", "small", "s9_1_4", "s9_2_3", "s9_2_3_pre", "split", "solve7", "solve6_1", "solve6_2", "solve6_3")
DX = ("inside", "kernel", "roles")
JOSEPH = ("batch", "lds", "lds_pair", "tile", "strips")
LDS_SLOTS = ("gram_lds", "lit_lds", "tprod_lds", "solve_lds", "ug_lds", "fin_lds")
FORM_BATCHES = (1, 3, 8, 128)


def forms(emu, statics, ml, batch, n, pre, whole, combined, lit=1, F=200):
    out = (C.c_long * emu.lp_forms_len())()
    assert emu.lp_forms(ml, F, batch, statics, n, int(pre), int(whole), int(combined), int(lit), out) == 0
    v = list(out)
    d = dict(chol=CHOL[v[0]], gram=GRAM[v[1]], gram_grid=v[2], gram_finish=v[3], lit_batch=v[4], tprod=TPROD[v[5]], tprod_grid=v[6], solve=SOLVE[v[7]],
             split_nt=v[8], own_chol=v[9], dx=DX[v[10]], joseph=JOSEPH[v[11]], grid=tuple(v[12:16]), role_wgs=v[16])
    for i, slot in enumerate(LDS_SLOTS):   # (bytes, the kernel whose limit covers them | None)
        k = v[18 + 2 * i]
        d[slot] = (v[17 + 2 * i], emu.lp_kernel_name(k).decode() if k >= 0 else None)
    return d


def trunc_lds_doubles(ml):
    m = 6 * ((ml + 1) // 2 - 1)
    return m * (m | 1) + m + 8


def expected_forms(ml, B, n, pre, whole, combined, lit):
    """the rules as the launch functions of rvio_hip.hip held them before update_forms() (propagate_dev, update_local_dev, launch_solve,
    launch_ug_final, update_global_dev, augment_compose_dev), written out: NOT computed through launch_plan.h"""
    c6m, c6 = 6 * (ml - 1), 6 * n
    ldh, dd = c6m + 1, 24 + c6
    nt = (dd + 15) // 16
    npair = nt * (nt + 1) // 2
    e = dict(split_nt=0, own_chol=0, role_wgs=0, tprod_grid=0, lit_batch=0, gram_grid=1, gram_finish=0, dx="inside", chol="none", tprod="none")
    kern = dict.fromkeys(LDS_SLOTS)
    # share reduction
    gram_batch_fits = B > 1 and 8 * max(c6m * ldh, trunc_lds_doubles(ml)) <= 64 * 1024
    if B >= 128 and combined and gram_batch_fits:
        e["gram"] = "batch4" if c6m <= 63 else "batch6"
        kern["gram_lds"] = "gram_reduce_batch_kernel<4>" if c6m <= 63 else "gram_reduce_batch_kernel<6>"
        e["lit_batch"] = int(lit)
        if lit:
            kern["lit_lds"] = "lit_batch_kernel"
    else:
        chunk = 64 if B == 1 else 256
        e.update(gram="reduce", gram_grid=max(1, min(1024, (c6 * ldh + chunk - 1) // chunk)), gram_finish=int(combined))
        kern["gram_lds"] = "gram_reduce_kernel"
    if B == 1:
        NT = 4 if c6m <= 64 else 6 if c6m <= 96 else 8 if c6m <= 128 else 12
        if NT <= 6 and n >= 1:
            e["chol"] = "role"
        if 96 < c6m <= 192 and n >= 1:
            e["chol"] = "queue"
        if NT == 4:
            e["solve"] = "small" if pre else "s9_1_4"
            e["dx"] = "roles" if pre and whole else "inside"
            if pre:
                kern["solve_lds"] = "solve9_small_kernel"
        elif NT == 6:
            e["solve"] = "s9_2_3_pre" if pre else "s9_2_3"
            e["dx"] = "roles" if whole else "inside"
        else:
            e.update(solve="split", split_nt=NT, own_chol=int(not pre), dx="roles" if whole and c6 > 64 else "kernel")
        if whole and c6 <= 60:
            e.update(joseph="lds", grid=(npair, 0, 0, 0))
            kern["ug_lds"] = "joseph_lds_kernel"
        elif c6 <= 64:
            e.update(joseph="lds_pair", grid=(nt, (npair + 3) // 4, 0, 0))
            kern["ug_lds"], kern["fin_lds"] = "ug_lds_kernel", "final_lds_kernel"
        else:
            c6t = (c6 + 15) // 16
            e.update(joseph="tile", grid=((nt * c6t + 3) // 4, (nt * c6t + 3) // 4, (nt * nt + 3) // 4, npair))
    else:
        if c6m > 126:
            e["solve"] = "solve7"
        else:
            v = 1 if c6m <= 60 else 2 if c6m <= 96 else 3
            e["solve"] = "solve6_%d" % v
            kern["solve_lds"] = ("solve6_kernel<1, 8, 8>", "solve6_kernel<2, 12, 8>", "solve6_kernel<2, 16, 8>")[v - 1]
            if B >= 128 and c6m <= 64:
                e["tprod"] = "gemm_lds"
                kern["tprod_lds"] = "gemm_T_lds_kernel"
            else:
                e.update(tprod="gemm", tprod_grid=(c6 + 31) // 32)
        if B >= 128 and c6m <= 60 and whole:
            e.update(joseph="batch", grid=(1, 0, 0, 0))
            kern["ug_lds"] = "joseph_batch_kernel"
        else:
            e.update(joseph="strips", grid=((dd + 15) // 16, (npair + 3) // 4, 0, 0))
            kern["ug_lds"] = "ug_kernel"
    if e["dx"] == "roles":
        e["role_wgs"] = (dd + 23) // 24
    return e, kern


def test_update_forms_for_every_window_and_clone_count(emu, statics, static_lds):
    seen = {k: set() for k in ("chol", "gram", "tprod", "solve", "dx", "joseph", "split", "lds_kernel")}
    for B in FORM_BATCHES:
        for ml in range(3, 33):
            p = evaluate(emu, statics, ml, 200, B)
            assert p["rc"] == 0 and p["lit_ok"] == 1
            for n in range(0, ml):
                c6, dd = 6 * n, 24 + 6 * n
                for pre in (0, 1):
                    for whole in (0, 1):
                        for combined in (0, 1):
                            f = forms(emu, statics, ml, B, n, pre, whole, combined)
                            at = (B, ml, n, pre, whole, combined)
                            # c. the parent's rules, both sides of every threshold (every n of every window is visited)
                            e, kern = expected_forms(ml, B, n, pre, whole, combined, 1)
                            for k, v in e.items():
                                assert f[k] == v, (at, k, f[k], v)
                            # a. roles only in a whole update, only where the Joseph launch has them, (24 + 6n + 23) / 24 of them
                            if f["dx"] == "roles":
                                assert whole and f["joseph"] in ("lds", "tile") and f["role_wgs"] == (dd + 23) // 24, at
                            else:
                                assert f["role_wgs"] == 0, at
                            assert not (whole and f["joseph"] == "lds_pair"), at      # (no window has 60 < 6n <= 64)
                            # b. every launch with dynamic LDS: bytes within the limit create_impl sets for the kernel it is budgeted under, which fits a CU
                            for slot in LDS_SLOTS:
                                nbytes, k = f[slot]
                                assert k == kern[slot], (at, slot, k, kern[slot])
                                if k is None:
                                    assert nbytes == 0, (at, slot)
                                    continue
                                assert nbytes > 0 or (k == "gemm_T_lds_kernel" and n == 0), (at, slot)
                                assert nbytes <= p["attr"][k] and p["attr"][k] + static_lds[k] <= LIMIT, (at, slot, nbytes, p["attr"][k])
                                seen["lds_kernel"].add(k)
                            # ... and the sizes the kernel files fix are used inside the windows they were fixed for
                            if f["joseph"] == "lds":
                                assert c6 <= 60 and f["ug_lds"][0] == (3 * 60 * 61 + 8 * 16 * 61 + 16) * 8, at
                            if f["joseph"] == "lds_pair":
                                assert c6 <= 64 and f["ug_lds"][0] == (2 * 64 * 65 + 88 * 65 + 2 * 16 * 65) * 8 and f["fin_lds"][0] == (3 * 88 * 65 + 4 * 16 * 17) * 8, at
                            if f["tprod"] == "gemm_lds":
                                assert f["tprod_lds"][0] == 2 * c6 * (c6 + 1) * 8 <= 2 * 64 * 65 * 8, at
                            if B < 128:
                                assert f["gram"] == "reduce" and f["tprod"] != "gemm_lds" and f["joseph"] != "batch", at
                            for k in ("chol", "gram", "tprod", "solve", "dx", "joseph"):
                                seen[k].add(f[k])
                            if f["solve"] == "split":
                                seen["split"].add((f["split_nt"], f["own_chol"]))
                        # d. sharded or not, one instance launches the same kernels: only the reduction's `finish` differs
                        if B == 1:
                            fa, fb = forms(emu, statics, ml, B, n, pre, whole, 1), forms(emu, statics, ml, B, n, pre, whole, 0)
                            assert (fa.pop("gram_finish"), fb.pop("gram_finish")) == (1, 0) and fa == fb, (ml, n, pre, whole)
    # every form was visited
    assert seen["chol"] == set(CHOL) and seen["gram"] == set(GRAM) and seen["tprod"] == set(TPROD) and seen["dx"] == set(DX) and seen["joseph"] == set(JOSEPH)
    assert seen["solve"] == set(SOLVE) - {"none"}
    assert seen["split"] == {(8, 0), (8, 1), (12, 0), (12, 1)}
    assert seen["lds_kernel"] == {"gram_reduce_kernel", "gram_reduce_batch_kernel<4>", "gram_reduce_batch_kernel<6>", "lit_batch_kernel", "gemm_T_lds_kernel",
                                  "solve9_small_kernel", "solve6_kernel<1, 8, 8>", "solve6_kernel<2, 12, 8>", "solve6_kernel<2, 16, 8>", "joseph_batch_kernel",
                                  "ug_kernel", "ug_lds_kernel", "final_lds_kernel", "joseph_lds_kernel"}


def test_update_form_thresholds(emu, statics):
    """single points on both sides of each threshold, as numbers (the sweep above checks the rule; this pins where it falls)"""
    def f1(ml, n, pre=1, whole=1, combined=1, B=1, lit=1):
        return forms(emu, statics, ml, B, n, pre, whole, combined, lit)
    # NT = 4 (6n_max <= 60), 6 (66..96), 8 (102..126), 12 (132..186)
    assert f1(11, 10)["solve"] == "small" and f1(11, 10, pre=0)["solve"] == "s9_1_4" and f1(11, 10, pre=0)["dx"] == "inside"
    assert f1(11, 10)["dx"] == "roles" and f1(11, 10, whole=0)["dx"] == "inside"
    assert f1(12, 11)["solve"] == "s9_2_3_pre" and f1(17, 16, pre=0)["solve"] == "s9_2_3" and f1(18, 17)["solve"] == "split"
    assert (f1(18, 17)["split_nt"], f1(22, 21)["split_nt"], f1(23, 22)["split_nt"], f1(32, 31)["split_nt"]) == (8, 8, 12, 12)
    assert f1(18, 17)["own_chol"] == 0 and f1(18, 17, pre=0)["own_chol"] == 1
    # the split solve's dx: its own launch while the window holds <= 10 clones (6n <= 64), roles from 11 on; always its own launch in a timed stage
    assert f1(18, 10)["dx"] == "kernel" and f1(18, 11)["dx"] == "roles" and f1(18, 11, whole=0)["dx"] == "kernel"
    # Joseph, one instance: 6n = 60 | 66
    assert f1(13, 10)["joseph"] == "lds" and f1(13, 11)["joseph"] == "tile" and f1(13, 10, whole=0)["joseph"] == "lds_pair" and f1(13, 11, whole=0)["joseph"] == "tile"
    assert f1(13, 10)["grid"][0] == 21 and f1(13, 10)["role_wgs"] == 4 and f1(13, 11)["role_wgs"] == 4 and f1(13, 12)["role_wgs"] == 4 and f1(17, 16)["role_wgs"] == 5
    # the Cholesky role
    assert [f1(ml, 1)["chol"] for ml in (3, 11, 12, 17, 18, 32)] == ["role", "role", "role", "role", "queue", "queue"]
    assert f1(11, 0)["chol"] == "none" and f1(18, 0)["chol"] == "none" and f1(11, 5, B=128)["chol"] == "none"
    # the reduction's grid: ceil(6n ldh / 64), at least 1, at most 1024
    assert (f1(11, 0)["gram_grid"], f1(11, 10)["gram_grid"], f1(32, 31)["gram_grid"]) == (1, 58, 544)
    assert f1(11, 10, B=8)["gram_grid"] == 15 and f1(11, 10, B=3)["gram"] == "reduce"
    # batches: the [A|b]-in-LDS reduction up to 6n_max = 90 (4 x 4 tiles up to 60), for >= 128 unsharded instances
    assert [f1(ml, 2, B=128)["gram"] for ml in (11, 12, 16, 17)] == ["batch4", "batch6", "batch6", "reduce"]
    assert f1(11, 2, B=128, combined=0)["gram"] == "reduce" and f1(11, 2, B=8)["gram"] == "reduce"
    assert f1(11, 2, B=128)["lit_batch"] == 1 and f1(11, 2, B=128, lit=0)["lit_batch"] == 0 and f1(17, 2, B=128)["lit_batch"] == 0
    # T product: in LDS up to 6n_max = 60 (<= 64), its own grid beyond, none behind solve7 (6n_max >= 132) and for one instance
    assert [f1(ml, 2, B=128)["tprod"] for ml in (11, 12, 22, 23)] == ["gemm_lds", "gemm", "gemm", "none"] and f1(11, 2, B=8)["tprod"] == "gemm"
    assert f1(12, 11, B=128)["tprod_grid"] == 3 and f1(11, 10)["tprod"] == "none"
    assert [f1(ml, 2, B=8)["solve"] for ml in (11, 12, 17, 18, 22, 23)] == ["solve6_1", "solve6_2", "solve6_2", "solve6_3", "solve6_3", "solve7"]
    # Joseph, batches
    assert f1(11, 10, B=128)["joseph"] == "batch" and f1(12, 10, B=128)["joseph"] == "strips" and f1(11, 10, B=128, whole=0)["joseph"] == "strips"
    assert f1(11, 10, B=8)["joseph"] == "strips" and f1(11, 10, B=8)["grid"][:2] == ((24 + 60 + 15) // 16, (6 * 7 // 2 + 3) // 4)


# ---------------------------------------------------------------- front_forms(): mode, synchronisation, stream roles and kernel forms of ONE front-end call
STREAM = ("filter", "tracker", "side", "image")
GRAY = ("none", "dword3", "byte3", "dword4", "byte4")
CLAHE_LUT = ("none", "col16_256x8", "col16_1024", "wave32")
CLAHE_INTERP = ("none", "px4", "px1")
PYRAMID = ("copy", "own")
DET_FIRST = ("none", "tile", "strip")
SUBPIX = ("none", "wide_win", "generic", "x16", "stock")
KLT = ("k3", "k16")
ANNOUNCE = ("none", "signal", "event")
BOOK = ("plain", "join", "fused", "pair")
FRONT_LAUNCHES = ("gray_l", "clahe_lut_l", "clahe_interp_l", "pyramid_l", "det_first_l", "neigh_l", "greedy_l", "subpix_l", "klt_l", "ransac_l", "book_a_l", "book_b_l")
FIXED_LDS = {-1: "none", -2: "default", -3: "neigh", -4: "greedy", -5: "subpix_wide"}
FRONT_DEFAULT = dict(throughput=0, W=752, H=480, equalizer=1, sp_win=7, channels=1, piped=1, have_list=0, frame_no=5, first_cleared=1, src_dword=1,
                     no_runahead=0, no_device_polls=0, own_queues=1)


def clahe_tiles(W, H):
    """createCLAHE(3.0, (5, 5)): a 5 x 5 tile grid over the image padded up to multiples of 5 (Tracker.cc:198-202)"""
    ew, eh = (W, H) if W % 5 == 0 and H % 5 == 0 else (W + 5 - W % 5, H + 5 - H % 5)
    return 5, 5, ew // 5, eh // 5


def front(emu, statics, ml, F, B, **kw):
    a = dict(FRONT_DEFAULT, **kw)
    tx, ty, tw, th = clahe_tiles(a["W"], a["H"]) if a["equalizer"] else (0, 0, 0, 0)
    vin = (a["throughput"], a["W"], a["H"], a["equalizer"], tx, ty, tw, th, a["sp_win"], a["channels"], a["piped"], a["have_list"], a["frame_no"],
           a["first_cleared"], a["src_dword"], a["no_runahead"], a["no_device_polls"], a["own_queues"])
    assert len(vin) == emu.lp_front_in_len()
    out = (C.c_long * emu.lp_front_len())()
    assert emu.lp_front_forms(ml, F, B, statics, (C.c_long * len(vin))(*vin), out) == 0
    v = list(out)
    keys = ("use_det", "piped", "runahead", "dev_sync", "par", "dslot", "ic", "lut_set", "det_set", "filter_done_by_counter", "wait_book_k3", "wait_first_flag",
            "pyr_on_image", "klt_polls_pyramid", "det_folds_signal", "fork_side")
    d = dict(zip(keys, v))
    k = len(keys)
    d["corners"] = ANNOUNCE[v[k]]
    for i, r in enumerate(("base", "image", "pyr", "side", "book")):
        d[r] = STREAM[v[k + 1 + i]]
    k += 6
    for i, (name, tab) in enumerate((("gray", GRAY), ("clahe_lut", CLAHE_LUT), ("clahe_interp", CLAHE_INTERP), ("pyramid", PYRAMID), ("det_first", DET_FIRST),
                                     ("subpix", SUBPIX), ("klt", KLT), ("book_form", BOOK))):
        d[name] = tab[v[k + i]]
    k += 8
    for i, name in enumerate(FRONT_LAUNCHES):   # (grid, threads, dynamic LDS, who covers it: a kernel of plan.attr | one of FIXED_LDS)
        gx, gy, gz, t, lds, kern = v[k + 6 * i: k + 6 * i + 6]
        d[name] = ((gx, gy, gz), t, lds, emu.lp_kernel_name(kern).decode() if kern >= 0 else FIXED_LDS[kern])
    return d


def cdiv(a, b):
    return (a + b - 1) // b


def expected_front(p, ml, F, B, a):
    """The front end's rules as DESIGN.md §3 and the comments at the launch sites state them, written out: NOT computed through launch_plan.h.
    p: the plan of the configuration (n_ic, book_fused, book_waves, book_lds); a: the call"""
    W, H, wide, eq = a["W"], a["H"], a["throughput"], a["equalizer"]
    e = {}
    # the pipelined whole-frame path with the device detector runs the front end in run-ahead form (unless RVIO_NO_RUNAHEAD); device-side counters for ONE
    # instance, unless stream events were asked for (RVIO_PARANOID) or a counter-collecting profiler serialises the queues
    det = not a["have_list"]
    ra = bool(a["piped"] and det and not a["no_runahead"])
    dev = ra and B == 1 and not a["no_device_polls"]
    k = a["frame_no"]
    par = k % 2 if a["piped"] else 0
    chain = k % p["n_ic"] if ra else 0                 # image chains exist in run-ahead mode only; the CLAHE LUTs alternate by parity outside it
    e.update(use_det=int(det), piped=a["piped"], runahead=int(ra), dev_sync=int(dev), par=par, dslot=k % 3 if ra else par, ic=chain, lut_set=chain if ra else par, det_set=chain)
    e["filter_done_by_counter"] = int(dev)
    e["wait_book_k3"] = int(ra and k >= 3)                                 # four equalised images, three corner lists in rotation: image chain k behind book-keeping(k-3)
    e["wait_first_flag"] = int(ra and k >= 1 and not a["first_cleared"])   # nms(k) behind book-keeping(k-1) until mbIsTheFirstImage is 0 everywhere
    on_image = bool(eq and ra)                                             # the pyramid rides on the image stream behind CLAHE
    polls = on_image and dev and a["own_queues"] and 6 * (ml - 1) <= 96 and not wide
    e.update(pyr_on_image=int(on_image), klt_polls_pyramid=int(polls), det_folds_signal=int(polls), fork_side=int(det and not on_image))
    e["corners"] = "signal" if dev else "event" if ra else "none"
    base = "tracker" if a["piped"] else "filter"
    e.update(base=base, image="image" if ra else base, side="side" if det else base, book="side" if ra else base)
    e["pyr"] = e["image"] if on_image else e["side"]
    # kernel forms
    L = {}
    no = ((0, 1, 1), 0, 0, "none")
    ch = a["channels"]
    if ch > 1:
        dword = W % 4 == 0 and a["src_dword"]
        e["gray"] = ("dword" if dword else "byte") + str(ch)
        L["gray_l"] = ((cdiv(W, 256), cdiv(H, 4), B), 256, 0, "none")
    else:
        e["gray"], L["gray_l"] = "none", no
    if eq:
        tx, ty, tw, th = clahe_tiles(W, H)
        col16 = cdiv(tw, 64) * th <= 65535                # a 16-bit counter sees one lane column of the tile
        e["clahe_lut"] = ("col16_256x8" if wide else "col16_1024") if col16 else "wave32"
        L["clahe_lut_l"] = ((tx * ty, 1, B), 256 if (wide and col16) else 1024, 0, "none")
        src_dword = W % 4 == 0 if ch > 1 else a["src_dword"]   # the handle's gray buffer: rows of W bytes, W H apart
        px4 = wide and W % 4 == 0 and src_dword
        e["clahe_interp"] = "px4" if px4 else "px1"
        L["clahe_interp_l"] = ((cdiv(W // 4, 64), cdiv(H, 16), B), 256, 0, "none") if px4 else ((cdiv(W, 64), cdiv(H, 4), B), 256, 0, "none")
    else:
        e["clahe_lut"], e["clahe_interp"], L["clahe_lut_l"], L["clahe_interp_l"] = "none", "none", no, no
    w3, h3 = W, H
    for _ in range(3):
        w3, h3 = (w3 + 1) // 2, (h3 + 1) // 2
    e["pyramid"] = "own" if eq else "copy"                # level 0 is the equalised image itself
    L["pyramid_l"] = ((cdiv(w3, 8), cdiv(h3, 8), B), 256, 0, "none")
    if det:
        e["det_first"] = "strip" if wide else "tile"
        L["det_first_l"] = ((cdiv(W, 60), cdiv(H, 16), B), 64, 0, "none") if wide else ((cdiv(W, 64), cdiv(H, 16), B), 512, 0, "none")
        L["neigh_l"] = ((2 if wide else 8, 1, B), 1024, 2048 * 18 + 4098 * 4, "neigh")
        L["greedy_l"] = ((1, 1, B), 1024, 4096 * 8 + 32768 + 24576 * 2 + 2052 * 4, "greedy")
        win = a["sp_win"]
        if win > 15:
            G = 64 if 2 * win + 1 <= 64 else 128
            e["subpix"], L["subpix_l"] = "wide_win", ((F, 1, B), 256, 8 * (5 * G * 17 + 5 * G + 8), "subpix_wide")
        elif win != 7:
            e["subpix"], L["subpix_l"] = "generic", ((F, 1, B), 256, 0, "none")
        elif wide:
            e["subpix"], L["subpix_l"] = "x16", ((cdiv(F, 4), 1, B), 64, 0, "none")
        else:
            e["subpix"], L["subpix_l"] = "stock", ((F, 1, B), 256, 0, "none")
    else:
        e["det_first"], e["subpix"] = "none", "none"
        L["det_first_l"] = L["neigh_l"] = L["greedy_l"] = L["subpix_l"] = no
    e["klt"] = "k16" if wide else "k3"
    L["klt_l"] = ((cdiv(F, 4) if wide else F, 1, B), 64, 0, "none")
    ransac = ((1, 1, B), 256, 8 * F + 16, "default")
    book_b = ((1, 1, B), 64 * p["book_waves"], p["book_lds"], "bookkeep_b_kernel")
    if not ra:
        e["book_form"] = "join" if det else "plain"
        bz = B if det else 1                               # the caller's list is ONE list: book-keeping of instance 0, one workgroup
        L.update(ransac_l=ransac, book_a_l=((1, 1, bz), 256, 0, "none"), book_b_l=((1, 1, bz),) + book_b[1:])
    elif dev and p["book_fused"]:
        e["book_form"] = "fused"
        L.update(ransac_l=((1, 1, B), 64 * p["book_waves"], p["book_lds"], "ransac_book_kernel"), book_a_l=no, book_b_l=no)
    else:
        e["book_form"] = "pair"
        L.update(ransac_l=ransac, book_a_l=no, book_b_l=book_b)
    e.update(L)
    return e


def check_front(emu, statics, static_lds, p, ml, F, B, a, seen):
    f = front(emu, statics, ml, F, B, **a)
    at = (ml, F, B, a)
    a = dict(FRONT_DEFAULT, **a)
    for k, v in expected_front(p, ml, F, B, a).items():
        assert f[k] == v, (at, k, f[k], v)
    # the invariants a change to one rule must not break
    assert (not f["dev_sync"] or f["runahead"]) and (not f["runahead"] or (f["use_det"] and f["piped"])), at
    if f["klt_polls_pyramid"]:
        assert f["dev_sync"] and a["equalizer"] and not a["throughput"] and 6 * (ml - 1) <= 96 and a["own_queues"], at
    assert bool(f["klt_polls_pyramid"]) == bool(f["det_folds_signal"]) and (not f["det_folds_signal"] or f["det_first"] == "tile"), at   # polled <=> a launch bumps it
    if f["book_form"] == "fused":
        assert f["dev_sync"] and p["book_fused"], at
    if f["piped"]:
        assert f["filter_done_by_counter"] == f["dev_sync"], at
    else:
        assert not f["filter_done_by_counter"], at
    assert 0 <= f["ic"] < p["n_ic"] and 0 <= f["dslot"] < 3 and 0 <= f["lut_set"] < max(2, p["n_ic"]) and 0 <= f["det_set"] < p["n_ic"], at
    # every launch: a workgroup the hardware takes, dynamic LDS within the limit that covers it
    for name in FRONT_LAUNCHES:
        (gx, gy, gz), t, lds, kern = f[name]
        if gx == 0:
            assert lds == 0 and kern == "none", (at, name)
            continue
        assert gx >= 1 and gy >= 1 and gz == (1 if name in ("book_a_l", "book_b_l") and f["book_form"] == "plain" else B) and 64 <= t <= 1024 and t % 64 == 0, (at, name, f[name])
        if kern == "none":
            assert lds == 0, (at, name)
        elif kern == "default":
            assert 0 < lds <= 64 * 1024, (at, name, lds)
        elif kern == "neigh":
            assert lds == emu.lp_neigh_lds() <= 64 * 1024, (at, name)
        elif kern == "greedy":
            assert lds == emu.lp_greedy_lds() <= LIMIT, (at, name)
        elif kern == "subpix_wide":
            assert lds == emu.lp_subpix_wide_lds_bytes(a["sp_win"]) <= LIMIT, (at, name)
        else:
            assert 0 < lds <= p["attr"][kern] and p["attr"][kern] + static_lds[kern] <= LIMIT, (at, name, lds, p["attr"][kern])
        seen["lds"].add(kern)
    for k in ("corners", "base", "image", "pyr", "side", "book", "gray", "clahe_lut", "clahe_interp", "pyramid", "det_first", "subpix", "klt", "book_form"):
        seen[k].add(f[k])
    seen["neigh"].add(f["neigh_l"][0][0])
    return f


def test_front_forms_for_every_mode_and_geometry(emu, statics, static_lds):
    seen = {k: set() for k in ("corners", "base", "image", "pyr", "side", "book", "gray", "clahe_lut", "clahe_interp", "pyramid", "det_first", "subpix", "klt",
                               "book_form", "neigh", "lds")}
    n = 0
    # a. the mode of a call: every combination of what it depends on, on both sides of 6n = 96 (windows 11, 17 | 18), F on both sides of the fused book-keeping launch
    for B in FORM_BATCHES:
        for ml, F in ((11, 200), (17, 200), (18, 200), (11, 3000)):
            p = evaluate(emu, statics, ml, F, B)
            assert p["rc"] == 0
            for eq in (0, 1):
                for thr in (0, 1):
                    for have_list in (0, 1):
                        for piped in (0, 1):
                            for no_ra in (0, 1):
                                for no_polls in (0, 1):
                                    for own in (0, 1):
                                        for first_cleared in (0, 1):
                                            for k in range(9):
                                                check_front(emu, statics, static_lds, p, ml, F, B, dict(equalizer=eq, throughput=thr, have_list=have_list, piped=piped,
                                                            no_runahead=no_ra, no_device_polls=no_polls, own_queues=own, first_cleared=first_cleared, frame_no=k), seen)
                                                n += 1
    # b. the kernel forms: image sizes (the third breaks the 16-bit histogram bound: tiles of 4096 x 1024, 64 lane columns x 1024 rows = 65 536), channel
    #    counts, alignment, cornerSubPix half-windows, for a run-ahead frame, a frame with a corner list and a per-stage call
    for B in FORM_BATCHES:
        p = evaluate(emu, statics, 11, 200, B)
        for W, H in ((752, 480), (1920, 1080), (20480, 5120), (750, 481)):
            for eq in (0, 1):
                for ch in (1, 3, 4):
                    for al in (0, 1):
                        for thr in (0, 1):
                            for win in (1, 7, 15, 16, 63):
                                for piped, have_list in ((1, 0), (1, 1), (0, 0)):
                                    check_front(emu, statics, static_lds, p, 11, 200, B, dict(W=W, H=H, equalizer=eq, channels=ch, src_dword=al, throughput=thr, sp_win=win,
                                                piped=piped, have_list=have_list), seen)
                                    n += 1
    print("front_forms: %d calls checked" % n)
    # every form, role and announcement was visited
    assert seen["corners"] == set(ANNOUNCE) and seen["gray"] == set(GRAY) and seen["clahe_lut"] == set(CLAHE_LUT) and seen["clahe_interp"] == set(CLAHE_INTERP)
    assert seen["pyramid"] == set(PYRAMID) and seen["det_first"] == set(DET_FIRST) and seen["subpix"] == set(SUBPIX) and seen["klt"] == set(KLT) and seen["book_form"] == set(BOOK)
    assert seen["base"] == {"filter", "tracker"} and seen["image"] == {"filter", "tracker", "image"} and seen["side"] == {"filter", "tracker", "side"}
    assert seen["pyr"] == set(STREAM) and seen["book"] == {"filter", "tracker", "side"} and seen["neigh"] == {0, 2, 8}
    assert seen["lds"] == {"none", "default", "neigh", "greedy", "subpix_wide", "bookkeep_b_kernel", "ransac_book_kernel"}


def test_front_form_thresholds(emu, statics):
    """single points on both sides of each threshold, by name (the sweep above checks the rule; this pins where it falls)"""
    def f1(ml=11, F=200, B=1, **kw):
        return front(emu, statics, ml, F, B, **kw)
    # run-ahead: a piped call with the device detector, unless RVIO_NO_RUNAHEAD; device-side counters: one instance, unless asked not to poll
    assert f1()["runahead"] and f1()["dev_sync"] and not f1(have_list=1)["runahead"] and not f1(piped=0)["runahead"] and not f1(no_runahead=1)["runahead"]
    assert f1(B=3)["runahead"] and not f1(B=3)["dev_sync"] and not f1(no_device_polls=1)["dev_sync"] and f1(no_device_polls=1)["runahead"]
    assert (f1()["corners"], f1(B=3)["corners"], f1(no_runahead=1)["corners"], f1(have_list=1)["corners"]) == ("signal", "event", "none", "none")
    # buffers in rotation: corner lists by frame % 3, image chains by frame % n_ic (two; ONE at 96 < 6n <= 192), else everything by parity
    assert [f1(frame_no=k)["dslot"] for k in range(6)] == [0, 1, 2, 0, 1, 2] and [f1(frame_no=k)["ic"] for k in range(4)] == [0, 1, 0, 1]
    assert [f1(ml=18, frame_no=k)["ic"] for k in range(4)] == [0, 0, 0, 0] and [f1(ml=17, frame_no=k)["ic"] for k in range(4)] == [0, 1, 0, 1]
    assert [(f1(have_list=1, frame_no=k)["dslot"], f1(have_list=1, frame_no=k)["lut_set"], f1(have_list=1, frame_no=k)["ic"]) for k in range(3)] == [(0, 0, 0), (1, 1, 0), (0, 0, 0)]
    assert [f1(piped=0, frame_no=k)["dslot"] for k in range(3)] == [0, 0, 0] and f1(no_runahead=1, frame_no=3)["det_set"] == 0 and f1(frame_no=3)["det_set"] == 1
    # the waits of the image chain: book-keeping(k-3) from frame 3 on, book-keeping(k-1) from frame 1 on until the first-image flag is gone
    assert [f1(frame_no=k)["wait_book_k3"] for k in (2, 3)] == [0, 1] and not f1(no_runahead=1, frame_no=5)["wait_book_k3"]
    assert [f1(frame_no=k, first_cleared=0)["wait_first_flag"] for k in (0, 1)] == [0, 1] and not f1(frame_no=5, first_cleared=1)["wait_first_flag"]
    # klt_kernel3 polls the pyramid counter: every term of the condition, one at a time
    assert f1()["klt_polls_pyramid"] and f1()["det_folds_signal"] and f1(ml=17)["klt_polls_pyramid"] and not f1(ml=18)["klt_polls_pyramid"]
    for off in (dict(equalizer=0), dict(throughput=1), dict(own_queues=0), dict(no_device_polls=1), dict(B=3), dict(no_runahead=1), dict(have_list=1), dict(piped=0)):
        assert not f1(**off)["klt_polls_pyramid"] and not f1(**off)["det_folds_signal"], off
    # where the pyramid runs, and who forks the side stream
    assert (f1()["pyr"], f1(equalizer=0)["pyr"], f1(no_runahead=1)["pyr"], f1(have_list=1)["pyr"], f1(piped=0, have_list=1)["pyr"]) == ("image", "side", "side", "tracker", "filter")
    assert (f1()["fork_side"], f1(equalizer=0)["fork_side"], f1(no_runahead=1)["fork_side"], f1(have_list=1)["fork_side"]) == (0, 1, 1, 0)
    assert (f1()["pyramid"], f1(equalizer=0)["pyramid"]) == ("own", "copy") and f1()["pyramid_l"][0] == (12, 8, 1) and f1(W=1920, H=1080)["pyramid_l"][0] == (30, 17, 1)
    # RANSAC / book-keeping: four shapes; the fused launch up to F = 2850 (one CU's LDS), with device-side counters only
    assert (f1()["book_form"], f1(F=2850)["book_form"], f1(F=2851)["book_form"], f1(B=3)["book_form"], f1(no_device_polls=1)["book_form"]) == ("fused", "fused", "pair", "pair", "pair")
    assert (f1(no_runahead=1)["book_form"], f1(have_list=1)["book_form"], f1(piped=0)["book_form"], f1(piped=0, have_list=1)["book_form"]) == ("join", "plain", "join", "plain")
    assert (f1()["book"], f1(no_runahead=1)["book"], f1(piped=0)["book"]) == ("side", "tracker", "filter")
    assert f1()["ransac_l"][1:] == (1024, 20 * 200 + 16 * 200 * 8 + 16, "ransac_book_kernel") and f1(B=3)["ransac_l"][1:] == (256, 1616, "default")
    assert f1(F=1600, ml=31)["ransac_l"][1] == 512 and f1(B=8)["book_b_l"][1] == 256
    # gray: dword form where W and the caller's base / strides are multiples of four
    assert (f1(channels=3)["gray"], f1(channels=3, src_dword=0)["gray"], f1(channels=4)["gray"], f1(channels=4, W=750)["gray"], f1()["gray"]) == ("dword3", "byte3", "dword4", "byte4", "none")
    assert f1(channels=3)["gray_l"][0] == (3, 120, 1) and f1(channels=3, B=8)["gray_l"][0] == (3, 120, 8)
    # CLAHE: 16-bit columns while ceil(tw / 64) * th <= 65535 — 20480 x 5115: 64 x 1023 = 65 472; 20480 x 5120: 64 x 1024 = 65 536; 1080p: 6 x 216
    assert (f1(W=20480, H=5115)["clahe_lut"], f1(W=20480, H=5120)["clahe_lut"], f1(W=1920, H=1080)["clahe_lut"]) == ("col16_1024", "wave32", "col16_1024")
    assert (f1(throughput=1)["clahe_lut"], f1(throughput=1)["clahe_lut_l"][1], f1()["clahe_lut_l"][1], f1(equalizer=0)["clahe_lut"]) == ("col16_256x8", 256, 1024, "none")
    assert (f1(throughput=1)["clahe_interp"], f1(throughput=1, src_dword=0)["clahe_interp"], f1(throughput=1, W=750)["clahe_interp"], f1()["clahe_interp"]) == ("px4", "px1", "px1", "px1")
    assert f1(throughput=1, channels=3, src_dword=0)["clahe_interp"] == "px4"      # (CLAHE then reads the handle's gray buffer, not the caller's image)
    assert f1(throughput=1)["clahe_interp_l"][0] == (3, 30, 1) and f1()["clahe_interp_l"][0] == (12, 120, 1)
    # detector: tile | strip first pass, 8 | 2 neighbour blocks; cornerSubPix: the stock window 7, other windows up to 15, the wide grid from 16 on (two sizes: 31 | 32)
    assert (f1()["det_first"], f1()["det_first_l"][0], f1(throughput=1)["det_first"], f1(throughput=1)["det_first_l"][0]) == ("tile", (12, 30, 1), "strip", (13, 30, 1))
    assert (f1()["neigh_l"][0][0], f1(throughput=1)["neigh_l"][0][0], f1(have_list=1)["neigh_l"][0][0]) == (8, 2, 0)
    assert [f1(sp_win=w)["subpix"] for w in (1, 6, 7, 8, 15, 16, 63)] == ["generic", "generic", "stock", "generic", "generic", "wide_win", "wide_win"]
    assert (f1(throughput=1)["subpix"], f1(throughput=1, sp_win=8)["subpix"], f1(throughput=1)["subpix_l"][0], f1(have_list=1)["subpix"]) == ("x16", "generic", (50, 1, 1), "none")
    assert (f1(sp_win=31)["subpix_l"][2], f1(sp_win=32)["subpix_l"][2]) == (46144, 92224)
    # KLT
    assert (f1()["klt"], f1()["klt_l"][0], f1(throughput=1)["klt"], f1(throughput=1)["klt_l"][0]) == ("k3", (200, 1, 1), "k16", (50, 1, 1))
