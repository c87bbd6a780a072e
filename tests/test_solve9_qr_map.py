"""solve9_small_kernel's Q / R phase deals its sixteen tiles to the sixteen waves by LP_S9SMALL_QR_MAP (launch_plan.h): tile (ti, tj) costs
(4 - tj) + (4 - ti) tile products, wave w runs on SIMD w & 3 — every tile must appear once and every SIMD must carry 20 of the 80 products."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _map():
    src = open(os.path.join(ROOT, "r-vio_amd", "csrc", "launch_plan.h")).read()
    v = int(re.search(r"#define\s+LP_S9SMALL_QR_MAP\s+(0x[0-9A-Fa-f]+)ull", src).group(1), 16)
    return [(v >> (4 * w)) & 15 for w in range(16)]


def test_every_tile_appears_once():
    assert sorted(_map()) == list(range(16))


def test_every_simd_gets_twenty_products():
    per_simd = [0, 0, 0, 0]
    for w, t in enumerate(_map()):
        ti, tj = t >> 2, t & 3
        per_simd[w & 3] += (4 - tj) + (4 - ti)
    assert per_simd == [20, 20, 20, 20]
    natural = [sum((4 - (w & 3)) + (4 - (w >> 2)) for w in range(16) if w & 3 == s) for s in range(4)]
    assert natural == [26, 22, 18, 14]          # what the map replaces
