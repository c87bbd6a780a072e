"""The short-window filter chain keeps its bits: set_state -> propagate -> update on a plain handle, against the oracle AND against what the
build before the solve / Joseph re-scheduling left for the same inputs (tests/golden/chain_bits_parent.npz, tools/record_chain_bits.py).

The re-scheduling (solve9.hip: the sweep's look-ahead factor, the pivot block of s9_factor from registers, the Q / R phase's wave-to-tile map;
joseph_lds_kernel at eight waves) moves work between waves and barrier intervals; every tile product keeps its operands and the order of its
MFMAs, every sum its order — so the results are the SAME BITS, not merely close.  cfg B (6n <= 60) takes solve9_small_kernel behind the
Cholesky role and joseph_lds_kernel with its dx roles; s9_factor is shared with the longer windows, which keep their bits too (cfg A:
solve9_kernel<2, 3, PRE>, cfg C: the split form)."""
import numpy as np
import pytest

import chain_bits_cases as CB
import oracle as O
import scenarios as S

abi = O.abi
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(CB.FIXTURE))


@pytest.fixture(scope="module")
def handles(gpu_required):
    from rvio_amd import hip
    hs = {}

    def get(cfg_name, cfg):
        if cfg_name not in hs:
            hs[cfg_name] = hip.RvioHip(cfg)
        return hs[cfg_name]
    yield get
    for h in hs.values():
        h.close()


def _check(case, g, handles):
    name = case[0]
    cfg, x0, P0, imu, types, lens, meas = CB.case_inputs(g, abi, case)
    x, P, err = CB.run_case(handles(case[1], cfg), x0, P0, imu, types, lens, meas)
    assert err == 0, name
    # the oracle, at the stage bars
    x1, P1 = O.propagate(cfg, x0, P0, imu)
    xo, Po, dg = O.update(cfg, x1, P1, types, lens, meas)
    assert bool(dg["updated"]) == (name != "pass"), name
    dx, dP, scale = S.state_delta(x, xo), float(np.max(np.abs(P - Po))), float(np.max(np.abs(Po)))
    print("%s: 6n = %d, |dx| %.2e, |dP| %.2e (max|P| %.2e)" % (name, 6 * ((len(x0) - 26) // 7), dx, dP, scale))
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(P)), name
    assert dx <= 1e-9 and dP <= 1e-9 * scale, name
    # the parent build's bits
    assert np.array_equal(x, g[name + "_x"]), name
    assert np.array_equal(P, P.T), name
    if name in CB.DIGEST_ONLY:
        assert CB.sha(P) == str(g[name + "_Psha"]), name
    else:
        assert np.array_equal(CB.triu(P), g[name + "_Pu"]), name


@pytest.mark.parametrize("case", CB.CASES_B, ids=[c[0] for c in CB.CASES_B])
def test_short_window_chain_keeps_the_parents_bits(case, fixture, handles):
    """cfg B: the window filling (n = 3, 5, 8: two, two and three tiles per side, each padded differently), the full window at its natural
    and at the headline load, the pass-through update (W = 0; the roles pass the state through) and a semi-definite clone block (the two
    newest clones with zero covariance: zero directions through s9_factor's pivot rule)"""
    _check(case, fixture, handles)


@pytest.mark.parametrize("case", CB.CASES_WINDOWS, ids=[c[0] for c in CB.CASES_WINDOWS])
def test_longer_windows_keep_the_parents_bits(case, fixture, handles):
    """cfg A (6n = 84, solve9_kernel<2, 3, PRE>) and cfg C (6n = 120, the split form) at full load: s9_factor is theirs too"""
    _check(case, fixture, handles)
