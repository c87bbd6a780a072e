"""CPU: the reader of rvio_replay --rel files (host/rvio_host.cpp parse_rels, through rvio_replay --check-rel): every kind by name and by number,
commas or blanks, the optional lever, and every malformed line refused with an error that names the file and the line.  And how the host
resolves a pair of stamps against the image stamps of the frames the clone window still reaches (resolve_rel_span, through rvio_replay
--check-rel-span): both stamps to the nearest frame, the newest image for a stamp at or past it, and the pairs that are dropped."""
import json
import subprocess

import pytest

from test_host import ensure_bin

STAMPS = "5.0,4.5,4.0,3.5"          # newest first: ages 0, 1, 2, 3
POSITION, ATTITUDE, POSE = 16, 17, 18


def check(tmp_path, text):
    p = tmp_path / "rels.txt"
    p.write_text(text)
    return subprocess.run([ensure_bin(), "--check-rel", str(p)], capture_output=True, text=True), str(p)


def test_good_file(tmp_path):
    r, _ = check(tmp_path, "# t_new t_old kind values sigmas [lever]\n"
                           "\n"
                           "2.5 2.0 position 0.1 -0.2 0.3  0.01 0.02 0.03\n"
                           "2.5, 2.0, 16, 0.1, -0.2, 0.3, 0.01, 0.02, 0.03, 0.3, -0.2, 0.1\r\n"
                           "   3.0 1.0 attitude 0 0.6 0 0.8  0.001 0.002 0.003\n"
                           "3.5 3.25 pose 1 2 3  0 0 0 1  0.1 0.2 0.3  0.01 0.02 0.03  0.5 0 -0.5\n"
                           "3.5 3.25 18 1 2 3  0 0 0 1  0.1 0.2 0.3  0.01 0.02 0.03\n"
                           "4.0 3.0 17 0 0 0 1  0.1 0.1 0.1\n")
    assert r.returncode == 0, r.stderr
    rows = [json.loads(l) for l in r.stdout.splitlines()]
    assert [(d["t_new"], d["t_old"], d["kind"]) for d in rows] == [(2.5, 2.0, POSITION), (2.5, 2.0, POSITION), (3.0, 1.0, ATTITUDE), (3.5, 3.25, POSE), (3.5, 3.25, POSE), (4.0, 3.0, ATTITUDE)]
    assert rows[0]["z"] == [0.1, -0.2, 0.3, 0, 0, 0, 0] and rows[0]["sigma"] == [0.01, 0.02, 0.03, 0, 0, 0] and rows[0]["lever"] == [0, 0, 0]
    assert rows[1]["z"] == rows[0]["z"] and rows[1]["sigma"] == rows[0]["sigma"] and rows[1]["lever"] == [0.3, -0.2, 0.1]
    assert rows[2]["z"] == [0, 0, 0, 0, 0.6, 0, 0.8] and rows[2]["sigma"] == [0, 0, 0, 0.001, 0.002, 0.003] and rows[2]["lever"] == [0, 0, 0]
    assert rows[3]["z"] == [1, 2, 3, 0, 0, 0, 1] and rows[3]["sigma"] == [0.1, 0.2, 0.3, 0.01, 0.02, 0.03] and rows[3]["lever"] == [0.5, 0, -0.5]
    assert rows[4]["z"] == rows[3]["z"] and rows[4]["lever"] == [0, 0, 0]


def test_empty_file_and_missing_file(tmp_path):
    r, _ = check(tmp_path, "# nothing\n\n")
    assert r.returncode == 0 and r.stdout == ""
    r = subprocess.run([ensure_bin(), "--check-rel", str(tmp_path / "absent.txt")], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot read" in r.stderr


@pytest.mark.parametrize("line,why", [
    ("2.5 2.0", "not `t_new t_old kind"),
    ("2.5 2.0 gravity 0 0 9.8 1 1 1", "unknown kind 'gravity'"),
    ("2.5 2.0 0 0.1 0.2 0.3 1 1 1", "unknown kind '0'"),
    ("2.5 2.0 19 0.1 0.2 0.3 1 1 1", "unknown kind '19'"),
    ("2.5 2.0 position 0.1 0.2 1 1 1", "position takes 3 values and 3 sigmas and an optional lever of 3"),
    ("2.5 2.0 position 0.1 0.2 0.3 1 1 1 0.1 0.2", "the line holds 8"),
    ("2.5 2.0 attitude 0 0 0 1 1 1 1 0.1 0.2 0.3", "attitude takes 4 values and 3 sigmas behind"),
    ("2.5 2.0 pose 1 2 3 0 0 0 1 1 1 1", "pose takes 7 values and 6 sigmas"),
    ("2.5 2.0 position 0.1 x 0.3 1 1 1", "'x' is not a finite number"),
    ("2.5 2.0 position 0.1 nan 0.3 1 1 1", "'nan' is not a finite number"),
    ("2.5 inf position 0.1 0.2 0.3 1 1 1", "'inf' is not a finite number"),
    ("2.5 2.0 position 0.1 0.2 0.3 1 0 1", "a sigma is not > 0"),
    ("2.5 2.0 pose 1 2 3 0 0 0 1 1 1 1 1 -1 1", "a sigma is not > 0"),
    ("2.5 2.0 attitude 0 0 0 1.1 1 1 1", "the quaternion is not of unit length"),
    ("2.0 2.5 position 0.1 0.2 0.3 1 1 1", "t_old is not before t_new"),
    ("2.5 2.5 position 0.1 0.2 0.3 1 1 1", "t_old is not before t_new"),
])
def test_a_malformed_line_is_an_error_that_names_the_line(tmp_path, line, why):
    r, path = check(tmp_path, "# header\n3.0 2.0 position 0 0 0 1 1 1\n" + line + "\n")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.startswith(path + ":3: ") and why in r.stderr and r.stderr.rstrip().endswith(line), r.stderr


# ---------------------------------------------------------------- the stamps
def span(t_new, t_old, stamps=STAMPS):
    r = subprocess.run([ensure_bin(), "--check-rel-span", stamps, repr(float(t_new)), repr(float(t_old))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    return (d["age_new"], d["age_old"]) if d["ok"] else None


@pytest.mark.parametrize("t_new,t_old,want", [
    (5.0, 4.5, (0, 1)), (5.0, 3.5, (0, 3)), (4.5, 4.0, (1, 2)), (4.0, 3.5, (2, 3)),
    (4.9, 4.4, (0, 1)), (4.76, 4.26, (0, 1)), (4.74, 4.24, (1, 2)),          # both to the NEAREST frame
    (4.75, 4.25, (1, 2)),                                                     # a tie goes to the older frame
    (4.6, 3.6, (1, 3)), (4.1, 3.5, (2, 3)),
    (5.0, 4.9, None), (4.6, 4.4, None), (3.6, 3.5, None),                      # both stamps on one frame
    (6.0, 4.5, (0, 1)), (7.5, 3.5, (0, 3)),                                    # at or past the newest composed image: age 0
    (6.0, 5.5, None), (6.0, 5.0, None), (6.0, 4.9, None),                      # ... both of them: one frame
    (5.0, 3.499, None), (4.5, -1.0, None), (3.4, 3.3, None),                   # the older stamp has left the window
])
def test_both_stamps_go_to_the_nearest_frame_or_the_pair_is_dropped(t_new, t_old, want):
    assert span(t_new, t_old) == want


def test_a_single_frame_and_no_frame():
    assert span(2.0, 1.9, stamps="2.0") is None and span(3.0, 2.0, stamps="2.0") is None
    assert span(2.0, 1.0, stamps="") is None
    assert span(2.0, 1.0, stamps="2.0,1.0") == (0, 1)


def test_replay_usage_lists_rel():
    usage = subprocess.run([ensure_bin()], capture_output=True, text=True)
    assert usage.returncode == 2 and "--rel FILE" in usage.stderr and "--rel-gate" in usage.stderr
