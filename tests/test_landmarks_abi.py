"""CPU-side checks of the landmark cloud's C-ABI surface (ABI 6): the entry points are exported and declared, they refuse a NULL
handle, and rvio_replay offers --landmarks.  No compute is launched here."""
import ctypes as C
import os
import re
import subprocess

import pytest

import oracle as O

abi = O.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_set_landmarks", "rvio_hip_get_landmarks", "rvio_hip_get_landmarks_at")


@pytest.fixture(scope="module")
def lib():
    from rvio_amd import build, hip
    build.build()
    return hip.load()


def test_abi_version_6_exports_the_cloud(lib):
    from rvio_amd import hip
    assert abi.ABI_VERSION == 6 and lib.rvio_hip_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    declared = set(re.findall(r"\b(rvio_(?:hip_)?[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in hip.SYMBOLS and hasattr(lib, s), s


def test_null_handle_is_invalid(lib):
    n, fr = C.c_int32(0), C.c_int32(0)
    assert lib.rvio_hip_set_landmarks(None, 1) == -1
    assert lib.rvio_hip_get_landmarks(None, C.byref(n), C.byref(fr), None, None, None) == -1
    assert lib.rvio_hip_get_landmarks_at(None, 0, C.byref(n), C.byref(fr), None, None, None) == -1


def test_replay_usage_lists_landmarks():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host")], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "host", "rvio_replay")], capture_output=True, text=True)
    assert r.returncode == 2 and "--landmarks FILE" in r.stderr, r.stderr
