"""The cases of tests/golden/meas_bits_parent.npz (test infrastructure).  Shared by tools/record_meas_bits.py, which writes the fixture, and
tests/test_gpu_meas_bits.py, which replays it: both run every case through the SAME run_case, so the bits recorded and the bits compared come
from identical calls.

A case is one handle of configuration B (leading dimension 84) that is given its state(s) and then takes one or two measurement updates —
auxiliary, standstill, absolute fix, past-frame fix — in their host or _dev form.  What the fixture holds:
    parent                     the commit whose build left the recorded outputs
    w<n>_x, w<n>_Pu, m<n>_x    the start states at n = 0, 3, 10 clones: aux_update_cases.window_state ('w') and fix_cases.moved_window ('m':
                               the same covariance), the covariance as its upper triangle
    <case>_<step>_<input>      the inputs of each step as raw bytes: H, v, sigma; imu; fix (records).  Modes, gates, instances, ages, fractions
                               and flags are those of the table below
    <case>_x<i>, <case>_Pu<i>  what the build left for instance i: the state in full, the covariance as its upper triangle
    <case>_<step>_<readback>   the feature's read-back behind each step, per instance: gamma / applied (aux_diag), rec (rvio_standstill,
                               rvio_fix_diag: raw bytes), rows_H / rows_sigma (get_fix_rows)
    <case>_err                 frame_info()["device_error"]
The generators (make_inputs) need the CPU oracle's recorded sequence; run_case needs the stored inputs and a device only."""
import os

import numpy as np

from pkgload import load_pkg

abi = load_pkg().abi
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "meas_bits_parent.npz")
WINDOWS = (0, 3, 10)
POSITION, ATTITUDE, POSE, GRAVITY = abi.RVIO_FIX_POSITION, abi.RVIO_FIX_ATTITUDE, abi.RVIO_FIX_POSE, abi.RVIO_FIX_GRAVITY
VALUE, RESIDUAL = abi.RVIO_AUX_VALUE, abi.RVIO_AUX_RESIDUAL
LEVER = (0.3, -0.2, 0.1)
SS_SAMPLES = 20


def aux(form, m, mode, gate=0, instance=-1, gamma=None, seed=0):
    """m = 3: aux_update_kernel<4>, m = 6: <16>.  host: one H for the instances `instance` names; dev: one per instance, each stride 5 doubles
    longer than its rows.  gamma (RESIDUAL): the residual is scaled to that chi-square value"""
    return dict(op="aux", form=form, m=m, mode=mode, gate=gate, instance=instance, gamma=gamma, seed=seed)


def ss(form, bias_rows, gate=0):
    """gate 0: the update is applied whatever the state's velocity (the window states are those of a platform in motion)"""
    return dict(op="ss", form=form, bias_rows=bias_rows, gate=gate)


def fix(form, kind, gate=0, instance=-1, active=None, seed=0):
    """host: one record; dev: one per instance (stride 1; a single instance: stride 0), active: None or the device flags"""
    return dict(op="fix", form=form, kind=kind, gate=gate, instance=instance, active=active, seed=seed)


def past(form, kind, age, frac=0.0, gate=0, instance=-1, active=None, seed=0):
    """age, frac: numbers (host), or one per instance (dev; an age > n lies outside the window)"""
    return dict(op="past", form=form, kind=kind, age=age, frac=frac, gate=gate, instance=instance, active=active, seed=seed)


def case(name, n, steps, states=("w",), filter_only=False):
    return dict(name=name, n=n, steps=steps, states=states, filter_only=filter_only or len(states) > 1)


CASES = [
    # auxiliary update, host form on every instance: both kernel forms, both modes, every window; the gate passing and refusing
    case("aux_h3_n0", 0, [aux("host", 3, VALUE)]), case("aux_h3_n3", 3, [aux("host", 3, VALUE, gate=1)]), case("aux_h3_n10", 10, [aux("host", 3, VALUE)]),
    case("aux_h6_n0", 0, [aux("host", 6, RESIDUAL, gate=1, gamma=100.0)]), case("aux_h6_n3", 3, [aux("host", 6, RESIDUAL)]),
    case("aux_h6_n10", 10, [aux("host", 6, RESIDUAL, gate=1, gamma=1.0)]),
    # ... on instance 1 of three (the staged flags are used, the other two stay as they are)
    case("aux_i3_n3", 3, [aux("host", 3, VALUE, instance=1)], states=("w", "m", "w")),
    case("aux_i6_n0", 0, [aux("host", 6, RESIDUAL, instance=1)], states=("w", "m", "w")),
    # ... the _dev form with per-instance strides
    case("aux_d3_n3", 3, [aux("dev", 3, VALUE)], states=("w", "m", "w")),
    case("aux_d6_n0", 0, [aux("dev", 6, RESIDUAL, gate=1, gamma=1.0)], states=("m", "w", "w")),
    # standstill on a filter-only handle, samples at rest, apply = 1
    case("ss_h0_n0", 0, [ss("host", 0, gate=1)], filter_only=True), case("ss_h1_n3", 3, [ss("host", 1)], filter_only=True),
    case("ss_d0_n0", 0, [ss("dev", 0)], filter_only=True), case("ss_d1_n3", 3, [ss("dev", 1)], filter_only=True),
    # absolute fixes: each kind in both forms; one _dev call with an instance switched off
    case("fix_h_pos_n3", 3, [fix("host", POSITION)], states=("m",)), case("fix_h_att_n0", 0, [fix("host", ATTITUDE, gate=1)], states=("m",)),
    case("fix_h_pose_n10", 10, [fix("host", POSE)], states=("m",)), case("fix_h_grav_n3", 3, [fix("host", GRAVITY)], states=("m",)),
    case("fix_d_pos_n0", 0, [fix("dev", POSITION)], states=("m",)), case("fix_d_att_n3", 3, [fix("dev", ATTITUDE)], states=("m",)),
    case("fix_d_pose_n3", 3, [fix("dev", POSE, active=(1, 0, 1))], states=("m", "w", "m")), case("fix_d_grav_n3", 3, [fix("dev", GRAVITY, gate=1)], states=("m",)),
    # past-frame fixes
    case("past_h_pos_n3", 3, [past("host", POSITION, 1, 0.4)], states=("m",)), case("past_h_pose_n3", 3, [past("host", POSE, 3)], states=("m",)),
    case("past_h_att_n10", 10, [past("host", ATTITUDE, 0)], states=("m",)), case("past_d_pos_n3", 3, [past("dev", POSITION, (1,), (0.4,))], states=("m",)),
    case("past_d_out_n3", 3, [past("dev", POSE, (0, 2, 4), (0.0, 0.0, 0.0))], states=("m", "w", "m")),
    # two host-form calls back to back on one handle: the second waits on the staging's event and allocates nothing
    case("twice_aux_n3", 3, [aux("host", 6, RESIDUAL, seed=1), aux("host", 3, VALUE, seed=2)]),
    case("twice_fix_n3", 3, [fix("host", POSE, seed=1), past("host", POSITION, 2, 0.4, seed=2)], states=("m",)),
]


def triu(P):
    return np.ascontiguousarray(P[np.triu_indices(P.shape[0])])


def from_triu(u):
    d = int(round((np.sqrt(8 * len(u) + 1) - 1) / 2))
    P = np.zeros((d, d))
    P[np.triu_indices(d)] = u
    return P + np.triu(P, 1).T


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()


def is_input(key):
    """a start state or a step's input (everything else in the fixture was left by the recorded build)"""
    return (key[0] in "wm" and key[1].isdigit()) or (key.endswith(("_H", "_v", "_sigma", "_imu", "_fix")) and "_rows_" not in key)


def config():
    return abi.config_named("B", enable_equalizer=0)


def states_of(g, c):
    P = from_triu(g["w%d_Pu" % c["n"]])
    return [(np.array(g["%s%d_x" % (v, c["n"])], float), P.copy()) for v in c["states"]]


# ---------------------------------------------------------------- inputs (the recorder's --inputs step; CPU)
def make_states():
    import aux_update_cases as A
    import fix_cases as F
    out = {}
    for n in WINDOWS:
        x, P = A.window_state(n)
        assert np.array_equal(P, P.T)
        out["w%d_x" % n], out["w%d_Pu" % n], out["m%d_x" % n] = x, triu(P), F.moved_window(n)[0]
    return out


def make_inputs(g, c):
    """-> {key: raw bytes} of every step of one case, from the generators of the feature tests"""
    import aux_update_cases as A
    import fix_cases as F
    import fix_past_cases as FP
    import standstill_cases as Z
    cfg, states, B, n, out = config(), states_of(g, c), len(c["states"]), c["n"], {}
    d = 24 + 6 * n
    for j, s in enumerate(c["steps"]):
        key = "%s_s%d_" % (c["name"], j)
        seed = 100 * s.get("seed", 0) + 10 * j
        if s["op"] == "aux":
            m, per = s["m"], (B if s["form"] == "dev" else 1)
            Hs, vs = np.zeros((per, m * d + 5)), np.zeros((per, m + 5))
            sg = np.ones((per, m + 5))
            for i in range(per):
                P = states[i if per > 1 else max(s["instance"], 0)][1]
                H, v, sigma = A.measurement(P, m, seed + i, "full", s["gamma"] if s["mode"] == RESIDUAL else None)
                if s["mode"] == VALUE:        # (xi is 0 in the rotation columns: the host form refuses an entry there)
                    H[:, [k for k in range(d) if k < 3 or 9 <= k < 12 or (k >= 24 and (k - 24) % 6 < 3)]] = 0.0
                Hs[i, :m * d], vs[i, :m], sg[i, :m] = H.reshape(-1), v, sigma
            out[key + "H"], out[key + "v"], out[key + "sigma"] = raw(Hs), raw(vs), raw(sg)
        elif s["op"] == "ss":
            out[key + "imu"] = raw(Z.imu_batch(states[0][0], SS_SAMPLES, seed=n, kind="rest"))
        elif s["op"] == "fix":
            per = B if s["form"] == "dev" else 1
            out[key + "fix"] = raw(np.concatenate([raw(np.frombuffer(bytes(F.fix_near(cfg, states[i][0], s["kind"], LEVER if i % 2 == 0 else (0.0, 0.0, 0.0), seed=seed + i)),
                                                                     np.uint8)) for i in range(per)]))
        else:
            per = B if s["form"] == "dev" else 1
            ages, fracs = (s["age"], s["frac"]) if s["form"] == "dev" else ((s["age"],), (s["frac"],))
            out[key + "fix"] = raw(np.concatenate([raw(np.frombuffer(bytes(FP.fix_near(states[i][0], s["kind"], min(ages[i], n), fracs[i], LEVER if i % 2 == 0 else (0.0, 0.0, 0.0),
                                                                                        sigma_p=0.02, sigma_q=0.005, seed=seed + i)), np.uint8)) for i in range(per)]))
    return out


# ---------------------------------------------------------------- the one run (recorder and test; GPU)
def _rec_bytes(r):
    return np.frombuffer(bytes(r), np.uint8).copy()


def run_case(g, c):
    """one handle, the stored inputs, every step -> {key: array} of everything the fixture holds for the case"""
    import torch
    from rvio_amd import hip
    import standstill_cases as Z
    name, n, B = c["name"], c["n"], len(c["states"])
    d = 24 + 6 * n
    states = states_of(g, c)
    h = hip.RvioHip(config(), batch=B, front_end=False) if c["filter_only"] else hip.RvioHip(config())
    keep = []

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        keep.append(t)
        return t.data_ptr()
    out = {}
    try:
        h.set_state(*states[0])                  # (the window length is handle-wide: set it, then the instances' own states)
        if B > 1:
            for i in range(B):
                h.set_state_at(i, *states[i])
        for j, s in enumerate(c["steps"]):
            key = "%s_s%d_" % (name, j)
            inp = lambda k, dt: np.ascontiguousarray(g[key + k]).view(dt)       # noqa: E731
            if s["op"] == "aux":
                m = s["m"]
                per = B if s["form"] == "dev" else 1
                H, v, sg = inp("H", np.float64).reshape(per, -1), inp("v", np.float64).reshape(per, -1), inp("sigma", np.float64).reshape(per, -1)
                if s["form"] == "host":
                    h.update_aux(H[0, :m * d].reshape(m, d), v[0, :m], sg[0, :m], s["mode"], s["gate"], s["instance"])
                else:
                    pH, pv, ps = dev(H), dev(v), dev(sg)
                    torch.cuda.synchronize()
                    h.update_aux_dev(m, s["mode"], s["gate"], pH, H.shape[1], pv, v.shape[1], ps, sg.shape[1], None)
                diag = [h.aux_diag(i) for i in range(B)]
                out[key + "gamma"], out[key + "applied"] = np.array([a[0] for a in diag]), np.array([a[1] for a in diag], np.int32)
            elif s["op"] == "ss":
                imu = inp("imu", abi.IMU_DTYPE)
                h.set_standstill(Z.ss_config(bias_rows=s["bias_rows"], gate=s["gate"]))
                if s["form"] == "host":
                    h.standstill(imu, 1)
                else:
                    p = dev(imu.view(np.uint8))
                    torch.cuda.synchronize()
                    h.standstill_dev(p, 0, len(imu), 1)
                out[key + "rec"] = np.stack([_rec_bytes(h.get_standstill(i)) for i in range(B)])
            else:
                recs = inp("fix", np.uint8).reshape(-1, 128)
                active = None if s["active"] is None else np.array(s["active"], np.int32)
                if s["form"] == "host":
                    f = abi.rvio_fix.from_buffer_copy(recs[0].tobytes())
                    if s["op"] == "fix":
                        h.update_fix(s["kind"], f, s["gate"], s["instance"])
                    else:
                        h.update_fix_past(s["kind"], f, s["age"], s["frac"], s["gate"], s["instance"])
                else:
                    pf, pa = dev(recs), (dev(active) if active is not None else None)
                    stride = 1 if len(recs) > 1 else 0
                    if s["op"] == "fix":
                        torch.cuda.synchronize()
                        h.update_fix_dev(s["kind"], s["gate"], pf, stride, pa)
                    else:
                        pg, pr = dev(np.array(s["age"], np.int32)), dev(np.array(s["frac"], np.float64))
                        torch.cuda.synchronize()
                        h.update_fix_past_dev(s["kind"], s["gate"], pf, stride, pg, pr, pa)
                out[key + "rec"] = np.stack([_rec_bytes(h.get_fix(i)) for i in range(B)])
                rows = [h.get_fix_rows(i) for i in range(B)]
                out[key + "rows_H"], out[key + "rows_sigma"] = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        for i in range(B):
            x, P = h.get_state_at(i) if B > 1 else h.get_state()
            out["%s_x%d" % (name, i)], out["%s_P%d" % (name, i)] = x, P
        out[name + "_err"] = np.array(h.frame_info()["device_error"])
    finally:
        h.close()
    return out
