"""The read window of the handle's record rings (csrc/ring_span.h: odometry ring, IMU-rate ring), compiled with g++ from
tests/hostemu/ring_span_emu.cpp and swept exhaustively on the CPU against a list model of the ring: capacity 1 .. 5, newest record 0 .. 3 cap + 1,
first_seq -2 .. newest + 2, record limit 0 .. cap + 2.  The model writes record seq (1-based) at slot (seq - 1) % cap, as the device does, and
reads the two spans back as the getters copy them."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "ring_span_emu.cpp")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ring_span") / "ring_span_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so])
    L = C.CDLL(so)
    LL = C.c_longlong
    L.rs_span.argtypes = [LL, LL, LL, LL, C.POINTER(LL)]
    L.rs_span.restype = None
    L.rs_slot.argtypes = [LL, LL]
    L.rs_slot.restype = LL
    L.rs_index.argtypes = [LL, LL, C.c_int, C.c_int]
    L.rs_index.restype = LL
    return L


def span(emu, newest, cap, first_seq, max_n):
    out = (C.c_longlong * 4)()
    emu.rs_span(newest, cap, first_seq, max_n, out)
    return tuple(out)     # first, count, slot0, n0


def sweep():
    for cap in range(1, 6):
        for newest in range(0, 3 * cap + 2):
            ring = [0] * cap          # slot -> the seq written there last (0: never written)
            for seq in range(1, newest + 1):
                ring[(seq - 1) % cap] = seq
            for first_seq in range(-2, newest + 3):
                for max_n in range(0, cap + 3):
                    yield cap, newest, ring, first_seq, max_n


def test_layout(emu):
    for cap in range(1, 6):
        for seq in range(1, 3 * cap + 2):
            assert emu.rs_slot(seq, cap) == (seq - 1) % cap
            for batch in (1, 3):
                for i in range(batch):
                    assert emu.rs_index(seq, cap, batch, i) == ((seq - 1) % cap) * batch + i


def test_every_window(emu):
    n = wrapped = 0
    for cap, newest, ring, first_seq, max_n in sweep():
        first, count, slot0, n0 = span(emu, newest, cap, first_seq, max_n)
        ctx = (cap, newest, first_seq, max_n)
        want = list(range(max(first_seq, newest - cap + 1, 1), newest + 1))[:max_n]
        # exactly the records the ring still holds from first_seq on, cut to max_n
        assert count == len(want), ctx
        if newest == 0:
            assert count == 0, ctx                     # nothing is served from an empty ring
        if count == 0:
            continue
        assert first == want[0], ctx
        n1 = count - n0
        assert 0 < n0 <= count and n1 >= 0, ctx        # first span + second span = the count
        assert 0 <= slot0 and slot0 + n0 <= cap, ctx
        if n1:
            assert slot0 + n0 == cap, ctx              # the second span (from slot 0) is empty unless the first ends at cap
            assert n1 <= slot0, ctx                    # ... and never runs into the first: at most one wrap
            wrapped += 1
        # read back as the getters copy: n0 records from slot0, the rest from slot 0 — consecutive seqs, each at slot (seq - 1) % cap
        slots = list(range(slot0, slot0 + n0)) + list(range(0, n1))
        assert [ring[s] for s in slots] == want, ctx
        assert slots == [(s - 1) % cap for s in want], ctx
        assert want == list(range(first, first + count)), ctx
        n += 1
    assert n > 1000 and wrapped > 100                  # (the sweep saw served windows, with and without a wrap)


def test_parent_formula_agrees(emu):
    """the arithmetic the two getters carried, written out as it stood: ring_span is a copy of it"""
    for cap, newest, ring, first_seq, max_n in sweep():
        lo = max(max(first_seq, newest - cap + 1), 1)
        cnt = max(0, min(newest - lo + 1, max_n))
        first, count, slot0, n0 = span(emu, newest, cap, first_seq, max_n)
        assert count == cnt
        if cnt:
            s0 = (lo - 1) % cap
            assert (first, slot0, n0) == (lo, s0, min(cnt, cap - s0))
