"""GPU: the FIRE kernels of include/ani_md.h (ani_md_fire_init / _iterate / _check) called directly through ctypes, against the
numpy FIRE of tests/fire_reference.py, one iteration at a time.  No model: forces are random numbers or a harmonic well.

Bars: dt, alpha and the counters exact; P, vv, ff within 1e-13 relative; x and v within 1e-13 of the largest |component| of the
reference array (fused multiply-adds on the device round differently, element by element a cancelling sum has no relative bar).
Sizes 1, 255, 256, 257 and 1500: a lone atom, a partial block, exactly one block, one block plus one atom, several blocks.
"""
import numpy as np
import pytest

import fire_reference as fr

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1500]
EXACT = ("iterations", "dt", "alpha", "last_negative", "uphill", "limited", "stop", "e_prev", "e_cur", "e_first")
REL = 1e-13


@pytest.fixture(scope="module")
def hip():
    from lammps_ani_amd import ani_hip
    return ani_hip


def _inputs(n, seed=0):
    rng = np.random.default_rng(1000 * seed + n)
    x = rng.uniform(0.0, 20.0, (n, 3))
    f = rng.normal(0.0, 15.0, (n, 3))
    m = fr.MASSES[rng.integers(0, 7, n)]
    return x, f, fr.FTM2V / m


class Device:
    """x, v, f, fm, ev, state and scratch on the card, and one ani_md_fire_iterate on them"""

    def __init__(self, hip, params, x, v, f, fm, E, state=None):
        import torch
        self.torch, self.hip, self.lib = torch, hip, hip.lib()
        dev = torch.device("cuda:0")
        self.n = n = x.shape[0]
        self.par = hip.fire_params(params["dt0"], params["etol"], params["ftol"], params["maxiter"],
                                   **{k: params[k] for k in params if k not in ("dt0", "etol", "ftol", "maxiter")})
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev).clone()
        self.x, self.v, self.f, self.fm = t(x), t(v), t(f), t(fm)
        self.xb = self.x.clone()
        self.ev = torch.zeros(10, dtype=torch.float64, device=dev)
        self.ev[0] = E
        self.d2max = torch.zeros(1, dtype=torch.float64, device=dev)
        self.state = torch.full((hip.FIRE_NSTATE,), 7.0, dtype=torch.float64, device=dev)
        self.work = torch.full((self.lib.ani_md_fire_work_size(n),), float("nan"), dtype=torch.float64, device=dev)
        assert self.lib.ani_md_fire_init(self.state.data_ptr(), self.v.data_ptr(), 0, self.par, None) == 0   # v kept
        if state:
            torch.cuda.synchronize()
            s = self.state.cpu().numpy()
            for k, val in state.items():
                s[hip.FIRE_STATE_KEYS.index(k)] = val
            self.state.copy_(torch.as_tensor(s))

    def iterate(self):
        rc = self.lib.ani_md_fire_iterate(self.x.data_ptr(), self.v.data_ptr(), self.f.data_ptr(), self.fm.data_ptr(), self.n,
                                          self.ev.data_ptr(), self.par, self.state.data_ptr(), self.work.data_ptr(),
                                          self.xb.data_ptr(), self.d2max.data_ptr(), None)
        assert rc == 0

    def read(self):
        self.torch.cuda.synchronize()
        return (self.x.cpu().numpy(), self.v.cpu().numpy(), dict(zip(self.hip.FIRE_STATE_KEYS, self.state.cpu().numpy().tolist())))


def _close(got, ref, what):
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f"  {what}: max |diff| {err:.3e} (largest |component| {scale:.3e})")
    assert err <= REL * max(scale, 1e-300), what


def _compare_state(got, ref):
    for k in EXACT:
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ("P", "vv", "ff", "ff_first", "dtv", "vmax"):
        assert abs(got[k] - ref[k]) <= REL * abs(ref[k]), (k, got[k], ref[k])


def _one_iteration(hip, n, params, v_of_f, E=-12.5, state=None, seed=0):
    """one iteration on the card and in numpy from the same inputs; returns the reference's verdict and both states"""
    x, f, fm = _inputs(n, seed)
    v = v_of_f(f)
    state = dict(state or {})
    ref = fr.Fire(params, fm)
    ref.set_state(**state)
    xr, vr = x.copy(), v.copy()
    what = ref.iterate(xr, vr, f, E)
    d = Device(hip, params, x, v, f, fm, E, state)
    d.iterate()
    xg, vg, sg = d.read()
    print(f"n {n} {what}: P {sg['P']:.6e} dt {sg['dt']} alpha {sg['alpha']} dtv {sg['dtv']:.6e} limited {sg['limited']}")
    _compare_state(sg, ref.state())
    _close(xg, xr, "x")
    _close(vg, vr, "v")
    d2 = ((xg - x) ** 2).sum(1).max()
    assert abs(float(d.d2max.cpu()[0]) - d2) <= 1e-13 * d2 + 1e-300      # the displacement maximum of the same pass
    return what, sg, ref


@pytest.mark.parametrize("n", SIZES)
def test_both_branches_and_the_start_from_rest(n, hip):
    p = fr.fire_defaults(0.5, 0.0, 0.0, 100, dmax=1e3)
    st = dict(iterations=4, dtv=0.4, e_prev=-12.0)
    what, s, _ = _one_iteration(hip, n, p, lambda f: 0.01 * f, state=st)
    assert what == "downhill" and s["uphill"] == 0 and s["P"] > 0
    what, s, _ = _one_iteration(hip, n, p, lambda f: -0.01 * f, state=st)
    assert what == "uphill" and s["uphill"] == 1 and s["last_negative"] == 5 and s["P"] < 0
    what, s, _ = _one_iteration(hip, n, p, lambda f: 0.0 * f)                       # iteration 1 of a run: the exact zero
    assert what == "uphill" and s["uphill"] == 1 and s["P"] == 0.0 and s["iterations"] == 1 and s["dt"] == 0.5
    # uphill after the delay, no half step back: alpha reset, dt halved
    p2 = fr.fire_defaults(0.5, 0.0, 0.0, 100, dmax=1e3, halfstepback=0, delaystep=3)
    what, s, _ = _one_iteration(hip, n, p2, lambda f: -0.01 * f, state=dict(iterations=4, dtv=0.4, alpha=0.2))
    assert what == "uphill" and s["dt"] == 0.25 and s["alpha"] == 0.25


@pytest.mark.parametrize("n", SIZES)
def test_dmax_limit_active_and_inactive(n, hip):
    x, f, fm = _inputs(n)
    vmax = np.abs(0.01 * f + (0.5 * fm)[:, None] * f).max()                          # roughly the move's largest velocity
    for dmax, limited in ((0.5 * vmax * 0.5, 1), (2.0 * vmax * 0.5, 0)):
        p = fr.fire_defaults(0.5, 0.0, 0.0, 100, dmax=dmax)
        what, s, ref = _one_iteration(hip, n, p, lambda f: 0.01 * f, state=dict(iterations=2, dtv=0.5))
        assert s["limited"] == limited and (s["dtv"] < 0.5) == bool(limited)


@pytest.mark.parametrize("n", SIZES)
def test_delaystep_just_reached_and_just_not(n, hip):
    p = fr.fire_defaults(0.5, 0.0, 0.0, 100, delaystep=5, dmax=1e3)
    # iteration k = 10: k - last_negative = 5 is not > delaystep, 6 is
    what, s, _ = _one_iteration(hip, n, p, lambda f: 0.01 * f, state=dict(iterations=9, last_negative=5, dtv=0.5))
    assert what == "downhill" and s["dt"] == 0.5 and s["alpha"] == 0.25
    what, s, _ = _one_iteration(hip, n, p, lambda f: 0.01 * f, state=dict(iterations=9, last_negative=4, dtv=0.5))
    assert what == "downhill" and s["dt"] == 0.5 * 1.1 and s["alpha"] == 0.25 * 0.99
    # growth stops at dtmax
    what, s, _ = _one_iteration(hip, n, p, lambda f: 0.01 * f, state=dict(iterations=9, last_negative=4, dtv=4.9, dt=4.9))
    assert s["dt"] == 5.0
    # an uphill event inside the initial delay keeps dt and alpha (k = 5 <= delaystep), the first one after it does not
    what, s, _ = _one_iteration(hip, n, p, lambda f: -0.01 * f, state=dict(iterations=4, alpha=0.2, dtv=0.5))
    assert what == "uphill" and s["dt"] == 0.5 and s["alpha"] == 0.2
    what, s, _ = _one_iteration(hip, n, p, lambda f: -0.01 * f, state=dict(iterations=5, alpha=0.2, dtv=0.5))
    assert what == "uphill" and s["dt"] == 0.25 and s["alpha"] == 0.25


@pytest.mark.parametrize("n", SIZES)
def test_dtshrink_refused_at_dtmin(n, hip):
    p = fr.fire_defaults(0.5, 0.0, 0.0, 100, dtmin=0.2, dmax=1e3)
    st = dict(iterations=30, last_negative=3, alpha=0.1, dtv=0.3)
    what, s, _ = _one_iteration(hip, n, p, lambda f: -0.01 * f, state=dict(st, dt=0.4))       # 0.2 >= dtmin: taken
    assert what == "uphill" and s["dt"] == 0.2 and s["alpha"] == 0.25
    what, s, _ = _one_iteration(hip, n, p, lambda f: -0.01 * f, state=dict(st, dt=0.39))      # 0.195 < dtmin: refused
    assert what == "uphill" and s["dt"] == 0.39 and s["alpha"] == 0.25


@pytest.mark.parametrize("n", SIZES)
def test_two_launches_give_bitwise_equal_sums(n, hip):
    x, f, fm = _inputs(n, seed=3)
    v = np.random.default_rng(n).normal(0.0, 0.05, (n, 3))
    p = fr.fire_defaults(0.5, 0.0, 0.0, 100)
    out = []
    for _ in range(2):
        d = Device(hip, p, x, v, f, fm, -3.0, dict(iterations=7, dtv=0.2))
        d.iterate()
        xg, vg, s = d.read()
        out.append((np.array([s["P"], s["vv"], s["ff"], s["dtv"], s["vmax"]]), xg, vg))
    for a, b in zip(out[0], out[1]):
        assert a.tobytes() == b.tobytes()


def _harmonic(n):
    rng = np.random.default_rng(42)
    x0 = rng.uniform(0.0, 20.0, (n, 3))
    kk = rng.uniform(200.0, 800.0, (n, 1))                      # kcal/mol/A^2: bond-like wells of different stiffness
    fm = fr.FTM2V / fr.MASSES[rng.integers(0, 7, n)]
    start = x0 + rng.normal(0.0, 0.08, (n, 3))
    return x0, kk, fm, start


HARMONIC = dict(n=257, params=fr.fire_defaults(0.5, 0.0, 1e-5, 5000))


def test_full_run_on_a_harmonic_well_stops_where_the_reference_stops(hip):
    import torch
    n, p = HARMONIC["n"], HARMONIC["params"]
    x0, kk, fm, start = _harmonic(n)
    ref = fr.Fire(p, fm)
    xr, hist = ref.run(lambda x: (-kk * (x - x0), float(0.5 * (kk * (x - x0) ** 2).sum())), start)
    assert ref.stop == 2 and 20 < ref.iterations < 3000
    d = Device(hip, p, start, np.zeros((n, 3)), np.zeros((n, 3)), fm, 0.0)
    x0d, kd = torch.as_tensor(x0, device=d.x.device), torch.as_tensor(kk, device=d.x.device)
    for _ in range(len(hist) + 10):                              # ten calls past the stop: frozen
        dx = d.x - x0d
        torch.mul(dx, -kd, out=d.f)
        d.ev[0] = 0.5 * (kd * dx * dx).sum()
        d.iterate()
    xg, vg, s = d.read()
    print(f"harmonic well: reference stops after {ref.iterations} iterations (code {ref.stop}), device after {int(s['iterations'])} "
          f"(code {int(s['stop'])}); max |dx| {np.abs(xg - xr).max():.3e}; uphill {int(s['uphill'])} / {ref.uphill}")
    assert s["iterations"] == ref.iterations and s["stop"] == ref.stop
    assert s["uphill"] == ref.uphill and s["limited"] == ref.limited and s["dt"] == ref.dt
    assert np.abs(xg - xr).max() < 1e-10


@pytest.mark.parametrize("code", [1, 2, 3, 4, "4f"])
def test_a_stopped_record_freezes_everything(code, hip):
    import torch
    n = 257
    x, f, fm = _inputs(n, seed=5)
    v = 0.01 * f
    E, st = -100.0, dict(iterations=30, last_negative=3, e_prev=-100.0 + 1e-7, dtv=0.3)
    if code == 1:
        p = fr.fire_defaults(0.5, 1e-6, 0.0, 100)
    elif code == 2:
        p = fr.fire_defaults(0.5, 0.0, 1e9, 100)
    elif code == 3:
        p = fr.fire_defaults(0.5, 0.0, 0.0, 30)
    elif code == 4:
        p, E = fr.fire_defaults(0.5, 0.0, 0.0, 100), float("nan")
    else:
        p = fr.fire_defaults(0.5, 0.0, 0.0, 100)
        f = f.copy()
        f[n // 2, 1] = float("inf")
    ref = fr.Fire(p, fm)
    ref.set_state(**st)
    xr, vr = x.copy(), v.copy()
    assert ref.iterate(xr, vr, f, E) == "stop" and ref.stop == (4 if code == "4f" else code)
    d = Device(hip, p, x, v, f, fm, E, st)
    d.iterate()
    xg, vg, s = d.read()
    assert s["stop"] == ref.stop and s["iterations"] == 30 and s["dt"] == 0.5 and s["e_prev"] == st["e_prev"]
    assert np.array_equal(xg, x) and np.array_equal(vg, v)                      # the stopping iteration does not move
    if ref.stop != 4:
        _compare_state(s, ref.state())
    state0 = d.state.cpu().numpy().copy()
    rng = np.random.default_rng(9)
    for _ in range(10):                                                         # new forces and energies: a live record would move
        d.f.copy_(torch.as_tensor(rng.normal(0.0, 15.0, (n, 3))))
        d.ev[0] = float(rng.normal())
        d.iterate()
    xg2, vg2, _ = d.read()
    assert xg2.tobytes() == x.tobytes() and vg2.tobytes() == v.tobytes()
    assert d.state.cpu().numpy().tobytes() == state0.tobytes()
    assert float(d.d2max.cpu()[0]) == 0.0


def test_check_brings_the_record_with_the_displacement_maximum(hip):
    import torch
    x, f, fm = _inputs(300)
    d = Device(hip, fr.fire_defaults(0.5, 0.0, 0.0, 100), x, 0.01 * f, f, fm, -1.0, dict(iterations=3))
    d.iterate()
    out = torch.zeros(1 + hip.FIRE_NSTATE, dtype=torch.float64, device=d.x.device)
    d2 = float(d.d2max.cpu()[0])
    assert d.lib.ani_md_fire_check(d.d2max.data_ptr(), d.ev.data_ptr(), d.state.data_ptr(), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert d2 > 0.0 and o[0] == d2 and float(d.d2max.cpu()[0]) == 0.0
    assert o[1:].tobytes() == d.state.cpu().numpy().tobytes() and o[1] == 4.0
    d.ev[0] = float("nan")
    d.lib.ani_md_fire_check(d.d2max.data_ptr(), d.ev.data_ptr(), d.state.data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    assert float(out.cpu()[0]) == float("inf")
