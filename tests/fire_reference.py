"""numpy FIRE, written from the contract of ani_md_fire_iterate in include/ani_md.h (LAMMPS `min_style fire`): the reference of
every FIRE test.  It takes any ``evaluate(x) -> (f, E)``.

`Fire.iterate` is one iteration on (x, v, f, E) and keeps the same state as the device record (`state()` returns it under the
names of ani_hip.FIRE_STATE_KEYS); `Fire.run` drives it with a calculator and records every iteration.  The oracle-driven
cases of the GPU tests (boxes, parameters) are defined here once, validated on the CPU by tests/test_fire_reference_cpu.py and
computed once per session (`oracle_case_run`).
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTM2V = 1.0 / 48.88821291 / 48.88821291   # LAMMPS units real, as lammps_ani_amd.md
MASSES = np.array([1.008, 12.011, 14.007, 15.999, 32.06, 18.998, 35.45])
STOP = ("running", "etol", "ftol", "maxiter", "non-finite")


def fire_defaults(dt0, etol, ftol, maxiter, **kw):
    p = dict(dt0=float(dt0), dtmax=10.0 * dt0, dtmin=0.02 * dt0, dtgrow=1.1, dtshrink=0.5, alpha0=0.25, alphashrink=0.99,
             delaystep=20, initialdelay=1, halfstepback=1, dmax=0.1, etol=float(etol), ftol=float(ftol), maxiter=int(maxiter))
    assert not set(kw) - set(p), sorted(set(kw) - set(p))
    p.update(kw)
    return p


class Fire:
    def __init__(self, params, fm):
        """params: fire_defaults(...); fm: per-atom ftm2v / mass [n]"""
        self.p = dict(params)
        self.fm = np.asarray(fm, dtype=np.float64)
        self.iterations, self.dt, self.alpha, self.last_negative = 0, self.p["dt0"], self.p["alpha0"], 0
        self.e_prev = self.e_cur = self.P = self.vv = self.ff = self.dtv = self.vmax = 0.0
        self.uphill = self.limited = self.stop = 0
        self.e_first = self.ff_first = 0.0

    def state(self):
        return dict(iterations=self.iterations, dt=self.dt, alpha=self.alpha, last_negative=self.last_negative, e_prev=self.e_prev,
                    e_cur=self.e_cur, P=self.P, vv=self.vv, ff=self.ff, dtv=self.dtv, uphill=self.uphill, limited=self.limited,
                    stop=self.stop, e_first=self.e_first, ff_first=self.ff_first, vmax=self.vmax)

    def set_state(self, **kw):
        for k, val in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, val)

    def iterate(self, x, v, f, E):
        """one iteration in place on x, v [n, 3]; returns what happened: 'frozen', 'stop', 'downhill' or 'uphill'"""
        p = self.p
        if self.stop != 0:
            return "frozen"
        P, vv, ff = float((v * f).sum()), float((v * v).sum()), float((f * f).sum())
        k = self.iterations + 1
        stop = 0
        if not (np.isfinite(E) and np.isfinite(ff)):
            stop = 4
        elif ff < p["ftol"] ** 2:
            stop = 2
        elif k > 1 and (k - 1 - self.last_negative) > p["delaystep"] and \
                abs(E - self.e_prev) < p["etol"] * 0.5 * (abs(E) + abs(self.e_prev) + 1e-8):
            stop = 1
        elif self.iterations == p["maxiter"]:
            stop = 3
        if stop:
            self.stop, self.e_cur, self.P, self.vv, self.ff = stop, float(E), P, vv, ff
            if self.iterations == 0:
                self.e_first, self.ff_first = float(E), ff
            return "stop"
        downhill = P > 0.0
        if downhill:
            s1 = 1.0 - self.alpha
            s2 = 0.0 if ff <= 1e-20 else self.alpha * np.sqrt(vv / ff)
            if k - self.last_negative > p["delaystep"]:
                self.dt = min(self.dt * p["dtgrow"], p["dtmax"])
                self.alpha *= p["alphashrink"]
        else:
            self.uphill += 1
            self.last_negative = k
            if not (p["initialdelay"] and k <= p["delaystep"]):
                self.alpha = p["alpha0"]
                if self.dt * p["dtshrink"] >= p["dtmin"]:
                    self.dt *= p["dtshrink"]
            if p["halfstepback"]:
                x -= 0.5 * self.dtv * v
            v[:] = 0.0
        v += (self.dt * self.fm)[:, None] * f
        if downhill:
            v[:] = s1 * v + s2 * f
        vmax = float(np.abs(v).max())
        dtv = self.dt
        if dtv * vmax > p["dmax"]:
            dtv = p["dmax"] / vmax
            self.limited += 1
        x += dtv * v
        self.dtv, self.vmax = dtv, vmax
        self.iterations, self.e_prev, self.e_cur, self.P, self.vv, self.ff = k, float(E), float(E), P, vv, ff
        if k == 1:
            self.e_first, self.ff_first = float(E), ff
        return "downhill" if downhill else "uphill"

    def run(self, evaluate, x0, max_calls=None):
        """iterate until a stop; returns (x, history): history[j] describes call j + 1 -- the state after it, what happened, the
        forces and energy it was given and the positions it left"""
        x = np.array(x0, dtype=np.float64)
        v = np.zeros_like(x)
        hist = []
        calls = 0
        while self.stop == 0 and (max_calls is None or calls < max_calls):
            f, E = evaluate(x)
            what = self.iterate(x, v, f, E)
            calls += 1
            hist.append(dict(self.state(), what=what, f=np.array(f), E=float(E), x=x.copy(), v=v.copy()))
        return x, hist


# ---- the oracle-driven cases of tests/test_fire_minimize.py -------------------------------------------------------------------------
# dt0, dtmax and delaystep were chosen on the CPU (tests/test_fire_reference_cpu.py checks what they have to give: an uphill event
# after iteration 1, a dt that grew, a dmax-limited move in one case, and |P| >= 0.05 sqrt(vv ff) wherever vv > 0, so that a
# rounding-level force difference cannot flip a branch).  etol = ftol = 0: the runs end by maxiter.
ORACLE_CASES = {
    "water30": dict(K=25, dt0=1.0, fire=dict(dtmax=4.0, delaystep=3)),                 # uphill at 13, one limited move (11)
    "water258": dict(K=12, dt0=4.0, fire=dict(dtmax=12.0, delaystep=1, dmax=0.5)),     # uphill at 5; long moves, none limited
}
_runs = {}


def case_system(name):
    from lammps_ani_amd import harness as hx
    if name == "water30":
        return hx.read_lammps_data(os.path.join(ROOT, "tests", "golden", "water-0.8nm.data"))
    return hx.spatial_sort(hx.water_box(258, seed=4))


def case_params(name):
    c = ORACLE_CASES[name]
    return fire_defaults(c["dt0"], 0.0, 0.0, c["K"], **c["fire"])


def oracle_evaluator(sysm, model_path):
    from lammps_ani_amd import harness as hx
    from oracle import Oracle
    o = Oracle(model_path)
    n = sysm.natoms

    def evaluate(xx):
        inp = hx.decompose(sysm, x_override=xx)
        r = o.compute(inp)
        f = np.zeros((n, 3))
        np.add.at(f, inp.tag[: inp.nlocal], r["force"][: inp.nlocal])
        np.add.at(f, inp.tag[inp.nlocal:], r["force"][inp.nlocal:])       # ghosts carry their owner's tag
        return f, r["energy"]

    return evaluate


def oracle_case_run(name, model_path):
    """the reference run of a case, computed once per process: (system, params, history)"""
    key = (name, model_path)
    if key not in _runs:
        sysm = case_system(name)
        fire = Fire(case_params(name), FTM2V / MASSES[sysm.types - 1])
        _, hist = fire.run(oracle_evaluator(sysm, model_path), sysm.x)
        _runs[key] = (sysm, case_params(name), hist)
    return _runs[key]
