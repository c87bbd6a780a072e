"""CPU: the reader of rvio_replay --fix files (host/rvio_host.cpp parse_fixes), through rvio_replay --check-fix: every kind by name and by
number, blanks or commas, comments and blank lines, the optional lever, the slots of rvio_fix each kind fills — and malformed lines, each refused
with an error that names the file and the line.  And the records the host hands to the library (tests/hostemu/fix_record_emu.cpp): the four
builders, the typed calls over them, and the queued fixes of a file, each byte for byte the rvio_fix written out here."""
import json
import os
import struct
import subprocess

import pytest

from test_host import ensure_bin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GOOD = """# t kind values... sigmas... [lever]

1.5 position 1 2 3  0.1 0.2 0.3
2.5, pose, 1,2,3, 0,0,0.6,0.8, 0.1,0.1,0.1, 0.01,0.02,0.03, 0.3,-0.2,0.1
3 1 0 0 0.6 0.8 0.01 0.01 0.02
4e0 gravity 0 9.8 0.1 .1 .1 .2
   5 0 1 2 3 0.5 0.5 0.5 0.3 -0.2 0.1
6 2 1 2 3 0 0 0 1 1 1 1 1 1 1
"""


def check(tmp_path, text):
    p = tmp_path / "fixes.txt"
    p.write_text(text)
    return subprocess.run([ensure_bin(), "--check-fix", str(p)], capture_output=True, text=True), str(p)


def test_good_file(tmp_path):
    r, _ = check(tmp_path, GOOD)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(l) for l in r.stdout.splitlines()]
    assert [x["t"] for x in rows] == [1.5, 2.5, 3.0, 4.0, 5.0, 6.0] and [x["kind"] for x in rows] == [0, 2, 1, 3, 0, 2]
    assert rows[0] == dict(t=1.5, kind=0, z=[1, 2, 3, 0, 0, 0, 0], sigma=[0.1, 0.2, 0.3, 0, 0, 0], lever=[0, 0, 0])
    assert rows[1] == dict(t=2.5, kind=2, z=[1, 2, 3, 0, 0, 0.6, 0.8], sigma=[0.1, 0.1, 0.1, 0.01, 0.02, 0.03], lever=[0.3, -0.2, 0.1])
    assert rows[2] == dict(t=3.0, kind=1, z=[0, 0, 0, 0, 0, 0.6, 0.8], sigma=[0, 0, 0, 0.01, 0.01, 0.02], lever=[0, 0, 0])
    assert rows[3] == dict(t=4.0, kind=3, z=[0, 9.8, 0.1, 0, 0, 0, 0], sigma=[0.1, 0.1, 0.2, 0, 0, 0], lever=[0, 0, 0])
    assert rows[4]["lever"] == [0.3, -0.2, 0.1] and rows[5]["lever"] == [0, 0, 0] and rows[5]["sigma"] == [1] * 6


def test_empty_file_and_missing_file(tmp_path):
    r, _ = check(tmp_path, "# nothing\n\n")
    assert r.returncode == 0 and r.stdout == ""
    r = subprocess.run([ensure_bin(), "--check-fix", str(tmp_path / "absent.txt")], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot read" in r.stderr


@pytest.mark.parametrize("line,why", [
    ("1.0 heading 0.3 0.01", "unknown kind 'heading'"),
    ("1.0 4 1 2 3 1 1 1", "unknown kind '4'"),
    ("1.0", "not `t kind"),
    ("1.0 position 1 2 3 0.1 0.1", "the line holds 5"),
    ("1.0 position 1 2 3 0.1 0.1 0.1 0.3 0.2", "the line holds 8"),
    ("1.0 attitude 0 0 0 1 0.1 0.1 0.1 0 0 0", "attitude takes 4 values and 3 sigmas behind"),
    ("1.0 gravity 0 0 9.8 0.1 0.1 0.1 0 0 0", "gravity takes 3 values and 3 sigmas behind"),
    ("1.0 pose 1 2 3 0 0 0 1 0.1 0.1 0.1", "pose takes 7 values and 6 sigmas"),
    ("1.0 position 1 2 x 0.1 0.1 0.1", "'x' is not a finite number"),
    ("1.0 position 1 2 nan 0.1 0.1 0.1", "'nan' is not a finite number"),
    ("1.0 position 1 2 3 0.1 inf 0.1", "'inf' is not a finite number"),
    ("1.0 position 1 2 3m 0.1 0.1 0.1", "'3m' is not a finite number"),
    ("t position 1 2 3 0.1 0.1 0.1", "'t' is not a finite number"),
    ("1.0 position 1 2 3 0.1 0 0.1", "a sigma is not > 0"),
    ("1.0 attitude 0 0 0 1 0.1 -0.1 0.1", "a sigma is not > 0"),
    ("1.0 attitude 0 0 0.1 1 0.1 0.1 0.1", "quaternion is not of unit length"),
    ("1.0 pose 1 2 3 0 0 0 0 1 1 1 1 1 1", "quaternion is not of unit length"),
])
def test_a_malformed_line_is_an_error_that_names_the_line(tmp_path, line, why):
    r, path = check(tmp_path, "# header\n1.5 position 1 2 3 0.1 0.2 0.3\n\n" + line + "\n2.0 gravity 0 0 9.8 1 1 1\n")
    assert r.returncode == 1 and r.stdout == "", (r.stdout, r.stderr)
    assert r.stderr.startswith(path + ":4: ") and why in r.stderr and r.stderr.rstrip().endswith(": " + line), r.stderr


# ---------------------------------------------------------------- the records the host hands to the library (tests/hostemu/fix_record_emu.cpp)
def record(z=(0,) * 7, sigma=(0,) * 6, lever=(0,) * 3):
    """rvio_fix as include/rvio_hip.h lays it out: z[7], sigma[6], lever[3], 128 bytes, no padding"""
    return struct.pack("<16d", *z, *sigma, *lever).hex()


# the values fix_record_emu.cpp hands to the builders and the typed calls, and the same fixes as lines of a file
P, Q, SP, SQ, LEVER, A = (1.0, -2.0, 3.5), (0.0, 0.6, 0.0, 0.8), (0.1, 0.2, 0.3), (0.01, 0.02, 0.03), (0.3, -0.2, 0.1), (0.0, 9.8, 0.1)
WANT = [(0, record(P + (0,) * 4, SP + (0,) * 3, LEVER)), (0, record(P + (0,) * 4, SP + (0,) * 3)), (1, record((0,) * 3 + Q, (0,) * 3 + SQ)),
        (2, record(P + Q, SP + SQ, LEVER)), (3, record(A + (0,) * 4, SP + (0,) * 3))]
LINES = """10 position 1 -2 3.5  0.1 0.2 0.3  0.3 -0.2 0.1
20 position 1 -2 3.5  0.1 0.2 0.3
30 attitude 0 0.6 0 0.8  0.01 0.02 0.03
40 pose 1 -2 3.5  0 0.6 0 0.8  0.1 0.2 0.3  0.01 0.02 0.03  0.3 -0.2 0.1
50 gravity 0 9.8 0.1  0.1 0.2 0.3
"""


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    ensure_bin()          # (the library and the host sources are built)
    tmp = tmp_path_factory.mktemp("fix_record")
    exe, fixes = tmp / "fix_record_emu", tmp / "fixes.txt"
    fixes.write_text(LINES)
    host, libdir = os.path.join(ROOT, "host"), os.path.join(ROOT, "r-vio_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", host, os.path.join(ROOT, "tests", "hostemu", "fix_record_emu.cpp"),
                           os.path.join(host, "rvio_host.cpp"), "-o", str(exe), "-L", libdir, "-lrvio_hip", "-lz", "-ldl",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    out = {}
    for line in subprocess.check_output([str(exe), str(fixes)], text=True).splitlines():
        tag, kind, hexbytes = line.split(" ")
        out.setdefault(tag, []).append((int(kind), hexbytes))
    return out


def test_each_builder_returns_the_record_of_its_kind(records):
    assert records["builder"] == WANT


def test_the_typed_calls_hand_on_the_builders_records(records):
    assert records["typed"] == WANT
    assert records["typed_past"] == WANT[:4]          # (GRAVITY has no past form)


def test_a_queued_fix_is_handed_on_as_the_typed_call_would_have_built_it(records):
    """System::apply_fixes passes the parsed record straight on: byte-equal to the typed call's, members the kind does not use included"""
    gravity = [w for w in WANT if w[0] == 3]
    assert records["queued"] == WANT + gravity        # without a latency all five; with one, GRAVITY alone is fused at the frame
    assert records["queued_past"] == WANT[:4]
    assert "unknown" not in records                   # a kind the parser never produces is refused, not handed on


def test_replay_usage_lists_fix():
    r = subprocess.run([ensure_bin()], capture_output=True, text=True)
    assert r.returncode == 2 and "--fix FILE" in r.stderr and "--fix-gate" in r.stderr, r.stderr
