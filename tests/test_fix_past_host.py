"""CPU: how the host resolves the stamp of a delayed fix against the image stamps of the frames the clone window still reaches
(host/rvio_host.cpp resolve_fix_age, through rvio_replay --check-fix-age): (age, frac) with interpolation for a position, the nearest frame for an
attitude or pose, snapping onto a frame, the fall-through at or past the newest image, the drop behind the oldest — and the parsing of
rvio_replay --fix-latency."""
import json
import subprocess

import pytest

from test_host import ensure_bin

STAMPS = "5.0,4.5,4.0,3.5"          # newest first: ages 0, 1, 2, 3
PAST, NOW, TOO_OLD = 0, 1, -1


def resolve(t, nearest=False, stamps=STAMPS):
    r = subprocess.run([ensure_bin(), "--check-fix-age", stamps, repr(float(t))] + (["nearest"] if nearest else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    return d["where"], d["age"], d["frac"]


@pytest.mark.parametrize("t,want", [
    (4.875, (PAST, 0, 0.25)), (4.5, (PAST, 1, 0.0)), (4.25, (PAST, 1, 0.5)), (4.0, (PAST, 2, 0.0)), (3.625, (PAST, 2, 0.75)), (3.5, (PAST, 3, 0.0)),
    (5.0, (NOW, 0, 0.0)), (5.2, (NOW, 0, 0.0)), (3.499, (TOO_OLD, 0, 0.0)), (-1.0, (TOO_OLD, 0, 0.0)),
])
def test_a_position_is_interpolated_between_the_two_frames_around_its_stamp(t, want):
    where, age, frac = resolve(t)
    assert (where, age) == want[:2] and abs(frac - want[2]) <= 1e-12 and 0.0 <= frac < 1.0


@pytest.mark.parametrize("t,want", [(4.5 - 1e-9, (1, 0.0)), (4.5 + 1e-9, (1, 0.0)), (4.0 + 1e-4, (1, 1.0 - 2e-4)), (4.0 - 1e-4, (2, 2e-4))])
def test_a_stamp_within_rounding_of_a_frame_snaps_onto_it(t, want):
    where, age, frac = resolve(t)
    assert where == PAST and age == want[0] and abs(frac - want[1]) <= 1e-9


@pytest.mark.parametrize("t,want", [(4.9, (PAST, 0)), (4.76, (PAST, 0)), (4.74, (PAST, 1)), (4.75, (PAST, 1)), (4.5, (PAST, 1)), (3.6, (PAST, 3)), (3.5, (PAST, 3)),
                                    (5.0, (NOW, 0)), (7.0, (NOW, 0)), (3.4, (TOO_OLD, 0))])
def test_an_attitude_or_pose_takes_the_nearest_frame(t, want):
    where, age, frac = resolve(t, nearest=True)
    assert (where, age) == want and frac == 0.0


def test_a_single_frame_and_no_frame():
    assert resolve(2.0, stamps="2.0") == (NOW, 0, 0.0) and resolve(1.9, stamps="2.0") == (TOO_OLD, 0, 0.0)
    assert resolve(1.0, stamps="") == (NOW, 0, 0.0)          # nothing composed yet: today's call decides (it refuses before initialisation)


def test_fix_latency_parsing():
    usage = subprocess.run([ensure_bin()], capture_output=True, text=True)
    assert usage.returncode == 2 and "--fix-latency S" in usage.stderr
    for bad in ("x", "-0.1", "nan", "inf", "0.1s", ""):
        r = subprocess.run([ensure_bin(), "settings.yaml", "root", "--fix", "f.txt", "--fix-latency", bad], capture_output=True, text=True)
        assert r.returncode == 1 and "--fix-latency takes seconds" in r.stderr, (bad, r.stderr)
    r = subprocess.run([ensure_bin(), "settings.yaml", "root", "--fix", "f.txt", "--fix-latency"], capture_output=True, text=True)
    assert r.returncode == 1 and "--fix-latency takes seconds" in r.stderr
    r = subprocess.run([ensure_bin(), "settings.yaml", "root", "--fix-latency", "0.1"], capture_output=True, text=True)
    assert r.returncode == 1 and "--fix-latency needs --fix" in r.stderr
    # a good value gets past the parser: the next complaint is about the settings file
    r = subprocess.run([ensure_bin(), "/nonexistent/settings.yaml", "root", "--fix", "f.txt", "--fix-latency", "0.15"], capture_output=True, text=True)
    assert r.returncode == 1 and "--fix-latency" not in r.stderr
