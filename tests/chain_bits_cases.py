"""The cases of tests/golden/chain_bits_parent.npz (test infrastructure, no oracle and no device here: numpy and the configuration table only).
Shared by tools/record_chain_bits.py, which writes the fixture, and tests/test_gpu_chain_bits.py, which replays it: both get every case's
inputs from the SAME function, so the bits recorded and the bits compared come from identical calls.

Every case is one set_state -> propagate -> update on a plain handle.  Keys of the fixture, per stored input set `s`:
    s_x0, s_P0u (upper triangle of the symmetric covariance), s_imu (raw bytes), s_types, s_lens, s_meas
(the full-load sets keep only s_imu: their state, covariance and tracks are those of tests/golden/full_load_inputs.npz, a fixture already)
and per case `c`:  c_x, and c_Pu (upper triangle: P+ leaves the Joseph form exactly symmetric, which the test asserts) or c_Psha (SHA-256)."""
import hashlib
import os
import sys

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "chain_bits_parent.npz")

# (case, configuration, stored input set, what is done to it)
CASES_B = [("fill3", "B", "fill3", None), ("fill5", "B", "fill5", None), ("fill8", "B", "fill8", None), ("n10", "B", "n10", None),
           ("full", "B", "full", None), ("pass", "B", "n10", "two_tracks"), ("zero", "B", "n10", "zero_newest_two")]
CASES_WINDOWS = [("winA", "A", "winA", None), ("winC", "C", "winC", None)]
DIGEST_ONLY = {"winA", "winC"}
FULL_LOAD_SETS = {"full": "B", "winA": "A", "winC": "C"}      # input set -> case of full_load_inputs.npz


def triu(P):
    return np.ascontiguousarray(P[np.triu_indices(P.shape[0])])


def from_triu(u):
    d = int(round((np.sqrt(8 * len(u) + 1) - 1) / 2))
    P = np.zeros((d, d))
    P[np.triu_indices(d)] = u
    return P + np.triu(P, 1).T


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_inputs(g, abi, case):
    """-> cfg, x0, P0, imu, types, lens, meas of one case, from the fixture g"""
    name, cfg_name, s, twist = case
    cfg = abi.config_named(cfg_name, enable_equalizer=0)
    imu = np.ascontiguousarray(g[s + "_imu"]).view(abi.IMU_DTYPE)
    if s in FULL_LOAD_SETS:             # a propagated state and its worst-case tracks behind one more propagation: that moves the IMU block only,
        sys.path.insert(0, GOLD)        # the tracks stay consistent with the clone poses
        import golden_io as M
        _, x0, P0, types, lens, meas = M.load_full_load_case(np.load(os.path.join(GOLD, "full_load_inputs.npz")), FULL_LOAD_SETS[s])
    else:
        x0, P0 = g[s + "_x0"].copy(), from_triu(g[s + "_P0u"])
        types, lens, meas = g[s + "_types"], g[s + "_lens"], g[s + "_meas"]
    if twist == "two_tracks":           # at most two features can be accepted: the pass-through update
        types, lens, meas = types[:2], lens[:2], meas[:2]
    elif twist == "zero_newest_two":    # a semi-definite clone block: the two newest clones with exactly zero covariance
        P0[-12:, :] = 0
        P0[:, -12:] = 0
    return cfg, x0, P0, imu, np.ascontiguousarray(types), np.ascontiguousarray(lens), np.ascontiguousarray(meas)


def run_case(h, x0, P0, imu, types, lens, meas):
    """the chain on a plain handle -> x, P, device_error"""
    h.set_state(x0, P0)
    h.propagate(imu)
    h.update(types, lens, meas)
    x, P = h.get_state()
    return x, P, h.frame_info()["device_error"]
