"""The launch forms of the pose-graph kernels (csrc/launch_plan.h window_edge_launch, window_joint_launch), compiled with g++ from
tests/hostemu/window_graph_plan_emu.cpp and checked on the CPU at batch 1 / 8 / 128 and every window: one workgroup of four waves per
(instance, pair) or (instance, age), no dynamic LDS, room for every column that is not zero at the longest span, and the kernels' static LDS —
read from the built library's gfx950 code object under the names launch_plan.h gives them — what the plan counts within the 160 KiB of a CU."""
import ctypes as C
import os
import subprocess

import pytest

from test_aux_plan import static_lds  # noqa: F401  (the fixture that reads the code object's notes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "window_graph_plan_emu.cpp")
LIMIT = 163840
EDGE, JOINT = "window_edge_kernel", "window_joint_kernel"


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("window_graph_plan") / "window_graph_plan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-variable", SRC, "-o", so])
    L = C.CDLL(so)
    L.wgp_kernel_name.restype = C.c_char_p
    for f in ("wgp_lds_limit", "wgp_chain_doubles", "wgp_edge_lds_doubles", "wgp_joint_lds_doubles", "wgp_pose_lds_doubles"):
        getattr(L, f).restype = C.c_long
    return L


def test_constants(emu):
    import window_cases
    abi = window_cases.abi
    assert emu.wgp_lds_limit() == LIMIT and emu.wgp_edge_threads() == 256 == emu.wgp_joint_threads()
    # the longest span the kernel's guard lets through: every clone of the longest chain
    assert emu.wgp_edge_nz() == 6 * emu.wgp_nmax() == 192 and emu.wgp_edge_nz() >= 6 * (emu.wgp_max_len() - 1)
    assert emu.wgp_edge_groups() * 36 <= emu.wgp_edge_threads()                   # one thread per (group, entry of the 6 x 6)
    assert 8 * emu.wgp_edge_words() == C.sizeof(abi.rvio_window_edge) == 376 and emu.wgp_edge_words() <= emu.wgp_edge_threads()
    assert emu.wgp_edge_max_pairs() == abi.WINDOW_EDGE_MAX_PAIRS == 528 == (emu.wgp_max_len() + 1) * emu.wgp_max_len() // 2
    assert emu.wgp_chain_doubles() == 12 * (emu.wgp_nmax() + 1)
    assert emu.wgp_edge_lds_doubles() == emu.wgp_chain_doubles() + 2 * 6 * emu.wgp_edge_nz() + 2 * 36 * emu.wgp_edge_groups() + emu.wgp_edge_words()
    # the joint kernel: what window_pose_kernel holds, the staged J_b and one order of the block's shares
    assert emu.wgp_joint_lds_doubles() == emu.wgp_pose_lds_doubles() + 6 * emu.wgp_pose_nz() + 36 * emu.wgp_pose_groups()
    names = [emu.wgp_kernel_name(k).decode() for k in range(emu.wgp_num_kernels())]
    assert names[emu.wgp_edge_id()] == EDGE and names[emu.wgp_joint_id()] == JOINT and len(set(names)) == len(names)


@pytest.mark.parametrize("batch", [1, 8, 128])
def test_one_workgroup_per_instance_and_pair_or_age(emu, batch):
    for max_len in range(3, 33):
        n = max_len - 1
        for cnt in (1, 2, n, n + 1, 528):
            out = (C.c_long * 6)()
            emu.wgp_edge_launch(batch, cnt, out)
            assert list(out) == [cnt, 1, batch, 256, 0, emu.wgp_edge_id()], (max_len, cnt)
        for cnt in (1, 2, n, n + 1):
            out = (C.c_long * 6)()
            emu.wgp_joint_launch(batch, cnt, out)
            assert list(out) == [cnt, 1, batch, 256, 0, emu.wgp_joint_id()], (max_len, cnt)
        assert 6 * n <= emu.wgp_edge_nz() and 6 + 6 * n <= emu.wgp_pose_nz()


@pytest.mark.parametrize("name", [EDGE, JOINT])
@pytest.mark.parametrize("batch", [1, 8, 128])
def test_static_lds_within_a_cu(emu, static_lds, batch, name):  # noqa: F811
    names = [emu.wgp_kernel_name(k).decode() for k in range(emu.wgp_num_kernels())]
    assert name in names and name in static_lds, name + " must be named in kLpKernelName and present in the built library"
    kern = names.index(name)
    st = static_lds[name]
    counted = 8 * (emu.wgp_edge_lds_doubles() if name == EDGE else emu.wgp_joint_lds_doubles())
    print("batch %d: static LDS of %s = %d B (the plan counts %d B), dynamic 0" % (batch, name, st, counted))
    # what the plan counts and alignment, nothing else
    assert counted <= st <= counted + 256 and st <= LIMIT
    # the plan sets no dynamic-LDS limit for it and accepts the stock handle with this static part ...
    statics = (C.c_size_t * len(names))(*[static_lds[nm] for nm in names])
    attr = C.c_long(-1)
    assert emu.wgp_plan(11, 200, batch, statics, kern, C.byref(attr)) == 0 and attr.value == 0
    # ... and refuses a build whose kernel would not fit a CU
    statics[kern] = LIMIT + 8
    assert emu.wgp_plan(11, 200, batch, statics, kern, C.byref(attr)) == 1
