"""The launch geometry of every accepted configuration, on the CPU.

rvio_hip_create / rvio_hip_create_batch accept max_track_len 3..32, n_features 2..4096 and any batch size; r-vio_amd/csrc/launch_plan.h derives
from them every dynamic-LDS size, the kernel variants and what moves from LDS to global memory, and create_impl applies exactly that text.
tests/hostemu/plan_emu.cpp compiles the same header with g++; this file sweeps EVERY window x EVERY feature count x batch in {1, 8, 128} and
checks, for every kernel that is given a dynamic-LDS limit, that dynamic + static fits the 163 840 B of a gfx950 CU — or that the plan refuses
the configuration with a message.  The static part is the compiler's decision: it is read from the BUILT library (the .hip_fatbin section ->
the gfx950 code object -> the kernel descriptors' notes), not from a table — the library must have been built (`__graft_entry__.build()`).

What this would have caught (and the arithmetic of the commit before it, kept here as `parent_book_lds`): book-keeping's LDS was budgeted
against 150 KB without ransac_book_kernel's 15 600 B of static LDS.  At n_features = 1024: 151 568 + 15 600 = 167 168 B; at 2851 (and every
larger count, batch handles included): 148 272 + 15 600 = 163 872 B — both beyond a CU, so such a handle failed with a HIP error.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostemu", "plan_emu.cpp")
HDR = os.path.join(ROOT, "r-vio_amd", "csrc", "launch_plan.h")
EMU = os.path.join(HERE, "hostemu", "libplan_emu.so")
LIB = os.path.join(ROOT, "r-vio_amd", "librvio_hip.so")
LIMIT = 163840
BATCHES = (1, 8, 128)


def _tool(name):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for p in (os.path.join(rocm, "llvm", "bin", name), os.path.join(rocm, "lib", "llvm", "bin", name), shutil.which(name) or ""):
        if p and os.path.exists(p):
            return p
    pytest.fail("%s not found (ROCm's LLVM tools are needed to read the built library's code object)" % name)


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
    if not os.path.exists(LIB):
        pytest.fail("r-vio_amd/librvio_hip.so has not been built: run __graft_entry__.build() first (this test reads the kernels' static LDS from it)")
    with tempfile.TemporaryDirectory() as t:
        fat, co = os.path.join(t, "fat.bin"), os.path.join(t, "gfx950.co")
        subprocess.check_call([_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", LIB, fat])
        subprocess.check_call([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--output=" + co,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"])
        notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    # one YAML map per kernel under amdhsa.kernels: its keys are sorted, .group_segment_fixed_size comes before .name
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\n\s*\.name:\s+(\S+)", blk)
        lds = re.search(r"\n\s*\.group_segment_fixed_size:\s+(\d+)", blk)
        assert name and lds, blk[:400]
        out[name.group(1)] = int(lds.group(1))
    assert len(out) > 40, "kernel descriptors not found in the code object's notes"
    dem = subprocess.run([shutil.which("c++filt") or _tool("llvm-cxxfilt")], input="\n".join(out), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(dem) == len(out)
    return {re.sub(r"\(.*", "", re.sub(r"^void ", "", d)): v for d, v in zip(dem, out.values())}


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
    attr, info, why = (C.c_size_t * n)(), (C.c_long * 16)(), C.create_string_buffer(256)
    rc = emu.lp_eval(ml, F, batch, statics, attr, info, why)
    keys = ("book_waves", "book_lds", "book_fused", "tm_global", "lit_state_global", "solve5_variant", "solve7_variant", "solve9_nt", "n_ic", "feat_threads",
            "feat_lds", "fprop_lds", "trunc_lds", "fuse_ok", "jb_lds", "gram_batch_lds")
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
