"""CPU: the reader of rvio_replay --map files (host/rvio_host.cpp parse_map, through rvio_replay --check-map): commas or blanks, comments, and
every malformed line refused with an error that names the file and the line.  How the host resolves a map stamp against the image stamps of the
frames the clone window still reaches (resolve_map_age, through rvio_replay --check-map-age): the nearest frame, the newest image for a stamp
at or past it, and the stamps that are skipped.  And the split of a group into calls of at most 8 points (map_calls, --check-map-split)."""
import json
import subprocess

import pytest

from test_host import ensure_bin

STAMPS = "5.0,4.5,4.0,3.5"          # newest first: ages 0, 1, 2, 3


def check(tmp_path, text):
    p = tmp_path / "map.txt"
    p.write_text(text)
    return subprocess.run([ensure_bin(), "--check-map", str(p)], capture_output=True, text=True), str(p)


def test_good_file(tmp_path):
    r, _ = check(tmp_path, "# t x y z u v sigma\n"
                           "\n"
                           "2.5 1.0 -2.0 3.0 320.5 240.25 1.5\n"
                           "2.5, 1.5, -2.5, 3.5, 100, 200, 0.5\r\n"
                           "   3.0 0 0 5 -0.1 0.2 0.004\n")
    assert r.returncode == 0, r.stderr
    rows = [json.loads(l) for l in r.stdout.splitlines()]
    assert [d["t"] for d in rows] == [2.5, 2.5, 3.0]
    assert rows[0]["p_w"] == [1.0, -2.0, 3.0] and rows[0]["uv"] == [320.5, 240.25] and rows[0]["sigma"] == 1.5
    assert rows[1]["p_w"] == [1.5, -2.5, 3.5] and rows[1]["uv"] == [100, 200] and rows[1]["sigma"] == 0.5
    assert rows[2]["p_w"] == [0, 0, 5] and rows[2]["uv"] == [-0.1, 0.2] and rows[2]["sigma"] == 0.004


def test_empty_file_and_missing_file(tmp_path):
    r, _ = check(tmp_path, "# nothing\n\n")
    assert r.returncode == 0 and r.stdout == ""
    r = subprocess.run([ensure_bin(), "--check-map", str(tmp_path / "absent.txt")], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot read" in r.stderr


@pytest.mark.parametrize("line,why", [
    ("2.5 1 2 3 100 200", "not `t x y z u v sigma`, the line holds 6 fields"),
    ("2.5 1 2 3 100 200 1.5 7", "the line holds 8 fields"),
    ("2.5 1 x 3 100 200 1.5", "'x' is not a finite number"),
    ("2.5 1 2 nan 100 200 1.5", "'nan' is not a finite number"),
    ("inf 1 2 3 100 200 1.5", "'inf' is not a finite number"),
    ("2.5 1 2 3 100 200 0", "sigma is not > 0"),
    ("2.5 1 2 3 100 200 -1.5", "sigma is not > 0"),
])
def test_a_malformed_line_is_an_error_that_names_the_line(tmp_path, line, why):
    r, path = check(tmp_path, "# header\n3.0 0 0 5 100 100 1\n" + line + "\n")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.startswith(path + ":3: ") and why in r.stderr and r.stderr.rstrip().endswith(line), r.stderr


# ---------------------------------------------------------------- the stamps
def age(t, stamps=STAMPS):
    r = subprocess.run([ensure_bin(), "--check-map-age", stamps, repr(float(t))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    return d["age"] if d["ok"] else None


@pytest.mark.parametrize("t,want", [
    (5.0, 0), (4.5, 1), (4.0, 2), (3.5, 3),                  # on a frame
    (4.9, 0), (4.76, 0), (4.74, 1), (4.3, 1), (4.2, 2),      # the NEAREST frame
    (4.75, 1),                                               # a tie goes to the older frame
    (5.01, 0), (7.5, 0),                                     # at or past the newest composed image: that image
    (3.499, None), (-1.0, None),                             # older than the window: skipped
])
def test_a_stamp_goes_to_the_nearest_frame_or_is_skipped(t, want):
    assert age(t) == want


def test_a_single_frame_and_no_frame():
    assert age(2.0, stamps="2.0") == 0 and age(3.0, stamps="2.0") == 0 and age(1.9, stamps="2.0") is None
    assert age(2.0, stamps="") is None


# ---------------------------------------------------------------- the split
@pytest.mark.parametrize("n,want", [(1, [[0, 1]]), (7, [[0, 7]]), (8, [[0, 8]]), (9, [[0, 8], [8, 1]]), (16, [[0, 8], [8, 8]]),
                                    (19, [[0, 8], [8, 8], [16, 3]]), (0, [])])
def test_more_than_eight_points_go_in_successive_calls(n, want):
    r = subprocess.run([ensure_bin(), "--check-map-split", str(n)], capture_output=True, text=True)
    assert r.returncode == 0 and json.loads(r.stdout) == want


def test_replay_usage_lists_map():
    usage = subprocess.run([ensure_bin()], capture_output=True, text=True)
    assert usage.returncode == 2 and "--map FILE" in usage.stderr and "--map-units px|norm" in usage.stderr and "--map-gate" in usage.stderr
