"""Inputs shared by the tests of the iterated measurement updates (test infrastructure): for each device-linearised family — an absolute
POSITION fix, a past-frame POSE fix, a REL_POSE between two frames, a stack of 8 map points — a measurement made AT a true state, and a prior
(x0, P0) that lies a known way off it: x0 = inject_state(x_true, delta), P0 = P + diag(delta_scale^2) on the perturbed columns.  `near` is
0.02 rad / 0.1 m, `far` 0.1 rad / 0.5 m.  The fix, past-fix and map cases perturb the qG and pG columns; a REL measurement does not read them,
so its case perturbs the clones of its span."""
import numpy as np

import map_cases as M

abi, A = M.abi, M.A
NEAR, FAR = (0.02, 0.1), (0.1, 0.5)
DIR_TH, DIR_P = np.array([0.8, -0.6, 0.7]), np.array([0.7, 0.5, -0.9])
SIGMA_P, SIGMA_Q = 0.01, 0.005          # metres, radians: the sigmas of the fix-family cases
FAMILIES = ("fix", "past", "rel", "map")
N, PAST_AGE, REL_SPAN, MAP_AGE = 10, 4, (2, 6), 4
CAL = M.calibrations()["radtan"]


class Case:
    """name, family, n, x_true, (x0, P0), lin(x, i) -> (H, r, sigma) — the family's row model, `i` the pass — and call(h, instance, gate): the
    same measurement through the handle's host entry point"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def model(self, max_iters, tol, dtype=float):
        self.reset()
        return abi.iter_update_model(self.x0, self.P0, self.lin, max_iters, tol, dtype)

    def one_shot(self):
        self.reset()
        return abi.aux_update_model(self.x0, self.P0, *self.lin(self.x0, 0))

    def whitened_ss(self, x):
        """the sum of squared whitened residuals of the measurement at the state x"""
        self.reset()
        _, r, s = self.lin(x, 0)
        return float(np.sum((r / s) ** 2))

    def reset(self):
        self.held = None


def _prior(x, P, scale, rot_cols, pos_cols):
    d = P.shape[0]
    delta, P0 = np.zeros(d), P.copy()
    for k, c in enumerate(rot_cols):
        sgn = 1.0 if k % 2 == 0 else -1.0      # (neighbouring clones turned opposite ways: the chain does not just rotate as a whole)
        delta[c: c + 3] = sgn * scale[0] * DIR_TH
        P0[c: c + 3, c: c + 3] += scale[0] ** 2 * np.eye(3)
    for k, c in enumerate(pos_cols):
        sgn = 1.0 if k % 2 == 0 else -1.0
        delta[c: c + 3] = sgn * scale[1] * DIR_P
        P0[c: c + 3, c: c + 3] += scale[1] ** 2 * np.eye(3)
    return abi.inject_state(x, delta), P0


def build(family, scale, n=N, age=None):
    cfg = A.long_config()
    xt, P = M.state(n)
    name = "%s-%s-n%d" % (family, "far" if scale == FAR else "near", n)
    c = Case(name=name, family=family, n=n, x_true=xt, held=None)
    if family == "rel":
        a, b = REL_SPAN
        clones = range(n - b, n - a)
        c.x0, c.P0 = _prior(xt, P, scale, [24 + 6 * i for i in clones], [27 + 6 * i for i in clones])
    else:
        c.x0, c.P0 = _prior(xt, P, scale, [0], [3])
    if family == "fix":
        lever = (0.3, -0.2, 0.1)
        fix = abi.make_fix(abi.fix_h(cfg, xt, abi.RVIO_FIX_POSITION, lever)[0:3], None, SIGMA_P, 0.0, lever)
        c.lin = lambda x, i: abi.fix_model(cfg, x, abi.RVIO_FIX_POSITION, fix)
        c.call = lambda h, instance=-1, gate=0: h.update_fix(abi.RVIO_FIX_POSITION, fix, gate, instance)
        c.rec = lambda h, i=0: h.get_fix(i)
    elif family == "past":
        age = PAST_AGE if age is None else age
        z = abi.fix_past_h(xt, age)
        fix = abi.make_fix(z[0:3], z[3:7], SIGMA_P, SIGMA_Q)
        c.lin = lambda x, i: abi.fix_past_model(x, abi.RVIO_FIX_POSE, fix, age)
        c.call = lambda h, instance=-1, gate=0: h.update_fix_past(abi.RVIO_FIX_POSE, fix, age, 0.0, gate, instance)
        c.rec = lambda h, i=0: h.get_fix(i)
    elif family == "rel":
        a, b = REL_SPAN
        z = abi.rel_h(xt, a, b)
        meas = abi.make_fix(z[0:3], z[3:7], SIGMA_P, SIGMA_Q)
        c.lin = lambda x, i: abi.rel_model(x, abi.RVIO_REL_POSE, meas, a, b)
        c.call = lambda h, instance=-1, gate=0: h.update_rel(abi.RVIO_REL_POSE, meas, a, b, gate, instance)
        c.rec = lambda h, i=0: h.get_fix(i)
    else:
        age = min(MAP_AGE, n) if age is None else age
        pts = M.observations(CAL, xt, age, [M.GOOD] * 8, seed=7)
        obs = abi.make_map_obs(pts)
        c.pts, c.age = pts, age

        def lin(x, i):
            # pass 0 decides the statuses (nothing is gated here: gate_each = 0), the later passes hold them
            H, r, s, g, st = abi.map_model(CAL, x, c.P0, obs, age, abi.RVIO_MAP_NORMALISED, 0, hold=None if i == 0 else c.held)
            c.held = (g, st) if i == 0 else (c.held[0], st)      # (a slot rejected at a later state stays rejected, as on the device)
            return H, r, s
        c.lin = lin
        c.call = lambda h, instance=-1, gate=0: h.update_map(obs, age, abi.RVIO_MAP_NORMALISED, gate, 0, instance)
        c.rec = lambda h, i=0: h.get_map(i)[0]
    return c


def cases():
    """every family near and far at n = 10"""
    return [build(f, s) for f in FAMILIES for s in (NEAR, FAR)]


def by_name(name):
    return {c.name: c for c in cases()}[name]
