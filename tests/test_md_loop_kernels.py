"""GPU: the time-step loop's kernels of include/ani_md.h -- integrators with the Langevin thermostat, ghost forward / reverse /
pack / unpack, gather / scatter, position wrap, ghost shell (count, scan, fill, append), displacement check -- called one at a
time through ctypes, against the numpy forms of tests/md_loop_reference.py.  Every test takes fresh device arrays, makes its
call, synchronises and compares.  No statistic is asserted here: the generator's moments and the thermostat's temperature are
asserted on the reference (tests/test_md_loop_reference_cpu.py), and the device is compared with the reference.

Bars of the integrators.  The reference evaluates every chain without fused multiply-adds; the device may fuse each one.  Both
results are the exact value perturbed by at most their own roundings, each rounding by 2^-53 of a partial result that the sum M
of the magnitudes of the chain's terms bounds.  With c roundings in the unfused chain, |device - reference| <= (2 c + 1) 2^-53 M:
c for either side, and one for the second-order terms and the rounding of M itself.  Counts c (propagated, DERIVED below):
    thermostat  f' = f + (g1 v + g2 r)        c = 4 (two products, two sums; r itself is exact),  M = |f| + |g1 v| + |g2 r|
    v' = v + s f                               c = 2 + c(f)                                        M = |v| + s M(f)
    v'' = v' + s f  (fused kernel)             c = 4 + c(f)                                        M = |v| + 2 s M(f)
    x' = x + dt v                              c = 2 + c(v)                                        M = |x| + dt M(v)
so c = 2 / 4 for initial_integrate's v / x, 4 / 6 for final_integrate's f / v with the thermostat (0 / 2 without), and
4 / 8 / 10 for the fused kernel's f / v / x with the thermostat (0 / 4 / 6 without).  No bar is looser than the 1e-13 of the
largest |component| that the FIRE and SHAKE tests use: the smaller of the two is applied per element.
d2max = max_i sum_k d_k^2 with d_k = x'_k - xb_k: |d_k| is off by at most bar(x'_k) + 2 2^-53 |d_k|, the three squares and
three sums (c = 5, all terms non-negative) add 11 2^-53 d2, and a maximum moves by no more than its largest element's error.

Ghost copies do one add or one copy per element, a single rounding that nothing can fuse: bit for bit.  The reverse kernels add
with atomics in no fixed order: their forces are multiples of 2^-20 bounded by 64, so that every partial sum is exact and the
result is bit-exact in any order.  Shell and check are integer- or bit-exact.  The wrap's bar is derived at its test.
"""
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

import md_loop_reference as mr
from test_md_loop_reference_cpu import COUNTER_EXAMPLES, _langevin_factors, free_particle_masses

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1500]
GHOSTS = [0, 1, 85, 86, 1500]            # 85 and 86 straddle one block of 256 threads at three threads per ghost
U = 2.0 ** -53
REL = 1e-13
SENTINEL = -7777.25
SEEDS_STEPS = [(12345, 0), (12345, 41), (0, 0), (0, 1 << 63), (1 << 63, (1 << 64) - 1), ((1 << 64) - 1, 1 << 63),
               ((1 << 64) - 1, (1 << 64) - 1), (1 << 63, 0)]
WORST = {}                                # kernel output -> largest |device - reference| / (2^-53 M) seen in this session


class Device:
    def __init__(self, hip):
        import torch
        self.torch, self.lib, self.dev = torch, hip.lib(), torch.device("cuda:0")

    def up(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a), device=self.dev).clone()

    def down(self, *tensors):
        self.torch.cuda.synchronize()
        return [t.cpu().numpy() for t in tensors]


@pytest.fixture(scope="module")
def dev():
    from lammps_ani_amd import ani_hip
    return Device(ani_hip)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _within(got, ref, count, mag, what):
    """|got - ref| <= (2 count + 1) 2^-53 mag per element, and no looser than REL of the largest |component|"""
    got, ref, mag = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(mag, dtype=np.float64)
    if ref.size == 0:
        assert got.size == 0
        return
    bar = np.minimum((2 * count + 1) * U * mag, REL * np.abs(ref).max())
    err = np.abs(got - ref)
    units = float((err / np.maximum(U * mag, 1e-300)).max())
    WORST[what] = max(WORST.get(what, 0.0), units)
    print(f"  {what}: largest error {units:.2f} x 2^-53 M (bar {2 * count + 1}), absolute {err.max():.3e}; worst so far {WORST[what]:.2f}")
    assert (err <= bar).all(), (what, float(err.max()), int(np.argmax(err - bar)))


def _same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    if got.tobytes() != ref.tobytes():
        bad = np.flatnonzero(got.ravel() != ref.ravel())
        raise AssertionError(f"{what}: {bad.size} elements differ, first at {bad[:5].tolist()}: "
                             f"{got.ravel()[bad[:5]].tolist()} against {ref.ravel()[bad[:5]].tolist()}")


# ---- integrators -----------------------------------------------------------------------------------------------------------
DT, TEMP, DAMP = 0.5, 300.0, 100.0


def _inputs(n, seed=0, tagged=False):
    from lammps_ani_amd import md
    rng = np.random.default_rng(1000 * seed + n)
    p = dict(x=rng.uniform(0.0, 20.0, (n, 3)), v=rng.normal(0.0, 0.01, (n, 3)), f=rng.normal(0.0, 15.0, (n, 3)))
    m = np.asarray(md.ANI2X_MASSES)[rng.integers(0, 7, n)]
    p["s"] = (0.5 * DT * md.FTM2V) / m
    p["g1"] = m * (-1.0 / DAMP / md.FTM2V)
    p["g2"] = np.sqrt(m) * ((24.0 * md.BOLTZ * TEMP / DAMP / DT / md.MVV2E) ** 0.5 / md.FTM2V)
    p["xb"] = p["x"] + rng.normal(0.0, 0.05, (n, 3))
    p["tags"] = (rng.permutation(n).astype(np.int64) + (1 << 33) + 7) if tagged else None    # a permutation, above 2^32
    return p


def _magnitudes(p, langevin, seed, step):
    """M and c of the module docstring for f', v' (one half kick), v'' (two) and x' = x + dt v''"""
    s = p["s"][:, None]
    if langevin:
        r = mr.draws(seed, step, np.arange(len(p["s"])) if p["tags"] is None else p["tags"])
        mf, cf = np.abs(p["f"]) + np.abs(p["g1"][:, None] * p["v"]) + np.abs(p["g2"][:, None] * r), 4
    else:
        mf, cf = np.abs(p["f"]), 0
    mv1, mv2 = np.abs(p["v"]) + s * mf, np.abs(p["v"]) + 2.0 * s * mf
    return dict(f=(cf, mf), v1=(cf + 2, mv1), v2=(cf + 4, mv2), x1=(cf + 4, np.abs(p["x"]) + DT * mv1),
                x2=(cf + 6, np.abs(p["x"]) + DT * mv2))


def _d2_bar(x_ref, xb, cx, mx):
    d = np.abs(x_ref - xb)
    per_atom = (2.0 * d * ((2 * cx + 1) * U * mx + 2.0 * U * d)).sum(1) + 11.0 * U * (d * d).sum(1)
    return float(per_atom.max()) if per_atom.size else 0.0


def _call_initial(D, p, d2max, n=None, x=None, v=None, f=None):
    t = [D.up(a) for a in (p["x"] if x is None else x, p["v"] if v is None else v, p["f"] if f is None else f, p["s"], p["xb"])]
    d = D.up(np.array([d2max]))
    n = len(p["s"]) if n is None else n
    assert D.lib.ani_md_initial_integrate(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), DT, n, t[4].data_ptr(),
                                          d.data_ptr(), None) == 0
    x, v, f, d = D.down(t[0], t[1], t[2], d)
    return x, v, f, d


def _call_final(D, p, langevin, seed, step, n=None):
    t = [D.up(a) for a in (p["v"], p["f"], p["s"], p["g1"], p["g2"])]
    tg = None if p["tags"] is None else D.up(p["tags"])
    n = len(p["s"]) if n is None else n
    assert D.lib.ani_md_final_integrate(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, langevin, t[3].data_ptr(), t[4].data_ptr(),
                                        _ptr(tg), seed, step, None) == 0
    return D.down(t[0], t[1])


def _call_fused(D, p, langevin, seed, step, d2max, n=None):
    t = [D.up(a) for a in (p["x"], p["v"], p["f"], p["s"], p["g1"], p["g2"], p["xb"])]
    tg = None if p["tags"] is None else D.up(p["tags"])
    d = D.up(np.array([d2max]))
    n = len(p["s"]) if n is None else n
    assert D.lib.ani_md_final_initial_integrate(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), DT, n, langevin,
                                                t[4].data_ptr(), t[5].data_ptr(), _ptr(tg), seed, step, t[6].data_ptr(), d.data_ptr(),
                                                None) == 0
    return D.down(t[0], t[1], t[2], d)


@pytest.mark.parametrize("n", SIZES)
def test_initial_integrate(n, dev):
    p = _inputs(n)
    x, v, f, d = _call_initial(dev, p, 0.0)
    xr, vr, dr = mr.initial_integrate(p["x"], p["v"], p["f"], p["s"], DT, p["xb"], 0.0)
    mg = _magnitudes(p, 0, 0, 0)
    _within(v, vr, *mg["v1"], "initial_integrate v")
    _within(x, xr, *mg["x1"], "initial_integrate x")
    _same(f, p["f"], "f is read only")
    bar = _d2_bar(xr, p["xb"], *mg["x1"])
    print(f"  d2max {d[0]!r} against {dr!r}: off by {abs(d[0] - dr):.3e}, bar {bar:.3e}")
    assert abs(d[0] - dr) <= bar


@pytest.mark.parametrize("tagged", [False, True], ids=["index", "tags"])
@pytest.mark.parametrize("langevin", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_final_integrate(n, langevin, tagged, dev):
    p = _inputs(n, 1, tagged)
    seed, step = 12345, 17
    v, f = _call_final(dev, p, langevin, seed, step)
    vr, fr = mr.final_integrate(p["v"], p["f"], p["s"], langevin, p["g1"], p["g2"], p["tags"], seed, step)
    mg = _magnitudes(p, langevin, seed, step)
    if langevin:
        _within(f, fr, *mg["f"], "final_integrate f")
    else:
        _same(f, p["f"], "f without the thermostat")
    _within(v, vr, *mg["v1"], "final_integrate v")


@pytest.mark.parametrize("tagged", [False, True], ids=["index", "tags"])
@pytest.mark.parametrize("langevin", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_fused_integrator_against_the_reference_and_bitwise_against_the_two_calls(n, langevin, tagged, dev):
    p = _inputs(n, 2, tagged)
    seed, step = 12345, (1 << 40) + 3
    x, v, f, d = _call_fused(dev, p, langevin, seed, step, 0.0)
    xr, vr, fr, dr = mr.final_initial_integrate(p["x"], p["v"], p["f"], p["s"], DT, p["xb"], 0.0, langevin, p["g1"], p["g2"], p["tags"],
                                                seed, step)
    mg = _magnitudes(p, langevin, seed, step)
    if langevin:
        _within(f, fr, *mg["f"], "final_initial_integrate f")
    else:
        _same(f, p["f"], "f without the thermostat")
    _within(v, vr, *mg["v2"], "final_initial_integrate v")
    _within(x, xr, *mg["x2"], "final_initial_integrate x")
    bar = _d2_bar(xr, p["xb"], *mg["x2"])
    print(f"  d2max {d[0]!r} against {dr!r}: off by {abs(d[0] - dr):.3e}, bar {bar:.3e}")
    assert abs(d[0] - dr) <= bar
    # "same arithmetic, same rounding as the two calls" (include/ani_md.h): bit for bit
    v1, f1 = _call_final(dev, p, langevin, seed, step)
    x2, v2, f2, d2 = _call_initial(dev, p, 0.0, v=v1, f=f1)
    _same(x, x2, "x of the fused kernel against the two calls")
    _same(v, v2, "v of the fused kernel against the two calls")
    _same(f, f2, "f of the fused kernel against the two calls")
    _same(d, d2, "d2max of the fused kernel against the two calls")


@pytest.mark.parametrize("fused", [False, True], ids=["final", "final_initial"])
@pytest.mark.parametrize("tagged", [False, True], ids=["index", "tags"])
@pytest.mark.parametrize("n", SIZES)
def test_thermostat_draws_are_the_reference_draws_bit_for_bit(n, tagged, fused, dev):
    """v = 0, f = 0, g2 = 1: the thermostat term g1 v + g2 r is exactly r, fused or not, and f after the call is the draw"""
    p = _inputs(n, 3, tagged)
    p["v"], p["f"], p["g2"] = np.zeros((n, 3)), np.zeros((n, 3)), np.ones(n)
    for seed, step in SEEDS_STEPS:
        f = _call_fused(dev, p, 1, seed, step, 0.0)[2] if fused else _call_final(dev, p, 1, seed, step)[1]
        r = mr.draws(seed, step, np.arange(n) if p["tags"] is None else p["tags"])
        _same(f, r, f"draws of seed {seed:#x} step {step:#x}")


D2_N = 1500
D2_SPOTS = {"atom 0": 0, "lane 63 of wave 3 of block 0": 255, "first atom of the last, partial block": 1280, "last atom": D2_N - 1}


@pytest.mark.parametrize("fused", [False, True], ids=["initial", "final_initial"])
@pytest.mark.parametrize("spot", sorted(D2_SPOTS))
def test_d2max_finds_the_largest_displacement_wherever_it_sits(spot, fused, dev):
    assert D2_N % 256 and D2_SPOTS["first atom of the last, partial block"] == (D2_N // 256) * 256
    p = _inputs(D2_N, 4)
    at = D2_SPOTS[spot]
    p["xb"][at] = p["x"][at] + np.array([0.9, -1.1, 0.7])                 # |d|^2 ~ 2.5 against ~ 0.0075 everywhere else
    if fused:
        x, _, _, d = _call_fused(dev, p, 0, 0, 0, 0.0)
        xr, _, _, dr = mr.final_initial_integrate(p["x"], p["v"], p["f"], p["s"], DT, p["xb"], 0.0)
        mg = _magnitudes(p, 0, 0, 0)["x2"]
    else:
        x, _, _, d = _call_initial(dev, p, 0.0)
        xr, _, dr = mr.initial_integrate(p["x"], p["v"], p["f"], p["s"], DT, p["xb"], 0.0)
        mg = _magnitudes(p, 0, 0, 0)["x1"]
    d2 = ((xr - p["xb"]) ** 2).sum(1)
    assert int(np.argmax(d2)) == at and d2[at] > 10.0 * np.delete(d2, at).max()
    bar = _d2_bar(xr, p["xb"], *mg)
    print(f"  {spot}: d2max {d[0]!r} against {dr!r}, off by {abs(d[0] - dr):.3e}, bar {bar:.3e}")
    assert abs(d[0] - dr) <= bar
    # a running maximum above every displacement stays as it is, bit for bit
    preset = float(np.nextafter(1.0e3, 2.0e3))
    d = (_call_fused(dev, p, 0, 0, 0, preset) if fused else _call_initial(dev, p, preset))[3]
    _same(d, np.array([preset]), "a preset maximum above every displacement")


@pytest.mark.parametrize("n", SIZES)
def test_d2max_at_every_size(n, dev):
    p = _inputs(n, 5)
    p["xb"][n - 1] = p["x"][n - 1] + np.array([-0.8, 0.6, 1.2])
    d = _call_initial(dev, p, 0.0)[3]
    xr, _, dr = mr.initial_integrate(p["x"], p["v"], p["f"], p["s"], DT, p["xb"], 0.0)
    assert abs(d[0] - dr) <= _d2_bar(xr, p["xb"], *_magnitudes(p, 0, 0, 0)["x1"])
    d = _call_fused(dev, p, 1, 9, 9, 0.0)[3]
    xr, _, _, dr = mr.final_initial_integrate(p["x"], p["v"], p["f"], p["s"], DT, p["xb"], 0.0, 1, p["g1"], p["g2"], None, 9, 9)
    assert abs(d[0] - dr) <= _d2_bar(xr, p["xb"], *_magnitudes(p, 1, 9, 9)["x2"])


def test_no_owned_atoms_touch_nothing(dev):
    p = _inputs(4, 6)
    x, v, f, d = _call_initial(dev, p, 3.5, n=0)
    for got, key in ((x, "x"), (v, "v"), (f, "f")):
        _same(got, p[key], key)
    _same(d, np.array([3.5]), "d2max")
    v, f = _call_final(dev, p, 1, 1, 1, n=0)
    _same(v, p["v"], "v"), _same(f, p["f"], "f")
    x, v, f, d = _call_fused(dev, p, 1, 1, 1, 3.5, n=0)
    for got, key in ((x, "x"), (v, "v"), (f, "f")):
        _same(got, p[key], key)
    _same(d, np.array([3.5]), "d2max")
    d = _call_initial(dev, _inputs(0), 0.0)[3]
    assert d[0] == 0.0


def test_integrators_leave_the_rows_behind_nlocal_alone(dev):
    """the owned block is the head of arrays that carry ghosts: nlocal = 257 of 300 rows"""
    p = _inputs(300, 7)
    n = 257
    x, v, f, d = _call_fused(dev, p, 1, 5, 6, 0.0, n=n)
    q = {k: (a[:n] if a is not None else None) for k, a in p.items()}
    xr, vr, fr, dr = mr.final_initial_integrate(q["x"], q["v"], q["f"], q["s"], DT, q["xb"], 0.0, 1, q["g1"], q["g2"], None, 5, 6)
    mg = _magnitudes(q, 1, 5, 6)
    _within(x[:n], xr, *mg["x2"], "final_initial_integrate x")
    _within(v[:n], vr, *mg["v2"], "final_initial_integrate v")
    for got, key in ((x, "x"), (v, "v"), (f, "f")):
        _same(got[n:], p[key][n:], key + " behind nlocal")
    assert abs(d[0] - dr) <= _d2_bar(xr, q["xb"], *mg["x2"])
    x, v, f, d = _call_initial(dev, p, 0.0, n=n)
    v2, f2 = _call_final(dev, p, 1, 5, 6, n=n)
    for got, key in ((x, "x"), (v, "v"), (f, "f"), (v2, "v"), (f2, "f")):
        _same(got[n:], p[key][n:], key + " behind nlocal")


def test_thermostat_trajectory_follows_the_reference(dev):
    """The free-particle recurrence of the CPU test (4096 atoms, 260 steps, factors from VerletRun._per_atom_factors) through
    ani_md_final_initial_integrate.  A step maps v to (1 - a) v + kick with 0 < 1 - a < 1: an error in v is handed on shrunk, so
    after k steps the device is within the SUM of the k single-step bars of the reference (c = 8 of the module docstring each)."""
    n, T, damp, dt, steps = 4096, 300.0, 10.0, 1.0, 260
    m = free_particle_masses(n)
    s, g1, g2 = _langevin_factors(m, T, damp, dt)
    tx, tv, tf = (dev.up(np.zeros((n, 3))) for _ in range(3))
    ts, tg1, tg2, txb = dev.up(s), dev.up(g1), dev.up(g2), dev.up(np.zeros((n, 3)))
    td = dev.up(np.array([1.0e300]))
    x, v, bar = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    worst = 0.0
    for step in range(steps):
        r = mr.draws(12345, step, np.arange(n))
        mf = np.abs(g1[:, None] * v) + np.abs(g2[:, None] * r)
        bar += (2 * 8 + 1) * U * (np.abs(v) + 2.0 * s[:, None] * mf)
        x, v, _, _ = mr.final_initial_integrate(x, v, np.zeros((n, 3)), s, dt, x, 0.0, 1, g1, g2, None, 12345, step)
        tf.zero_()
        assert dev.lib.ani_md_final_initial_integrate(tx.data_ptr(), tv.data_ptr(), tf.data_ptr(), ts.data_ptr(), dt, n, 1, tg1.data_ptr(),
                                                      tg2.data_ptr(), None, 12345, step, txb.data_ptr(), td.data_ptr(), None) == 0
        if step % 20 == 19 or step == steps - 1:
            (vd,) = dev.down(tv)
            err = np.abs(vd - v)
            worst = max(worst, float((err / bar).max()))
            assert (err <= bar).all(), (step, float(err.max()))
    print(f"  {steps} steps: largest |dv| / accumulated bar {worst:.3f}; final |dv| max {err.max():.3e} of |v| max {np.abs(v).max():.3e}")
    (d,) = dev.down(td)
    assert d[0] == 1.0e300


# ---- ghost kernels ---------------------------------------------------------------------------------------------------------
NLOCAL = 64
TAIL = 3            # rows behind everything a kernel may touch, pre-filled with the sentinel


def _owners(ng, layout, rng):
    """layout "mixed": owner 0 has no ghost, owner 1 one, owner 2 twenty-six (where ng allows), the rest fall at random on
    3 .. NLOCAL - 1;  "one": every ghost on owner 5"""
    if layout == "one":
        return np.full(ng, 5, dtype=np.int64)
    owner = rng.integers(3, NLOCAL, ng).astype(np.int64)
    fixed = np.array([1] + [2] * 26, dtype=np.int64)[:ng]
    owner[rng.permutation(ng)[:len(fixed)]] = fixed
    return owner


def _exact_forces(rng, rows):
    return rng.integers(-64 << 20, (64 << 20) + 1, (rows, 3)).astype(np.float64) * 2.0 ** -20


def _ghost_case(ng, layout, seed=0):
    rng = np.random.default_rng(100 * ng + seed + (7 if layout == "one" else 0))
    owner = _owners(ng, layout, rng)
    if layout == "mixed" and ng >= 27:
        cnt = np.bincount(owner, minlength=NLOCAL)
        assert cnt[0] == 0 and cnt[1] == 1 and cnt[2] == 26
    rows = NLOCAL + ng + TAIL
    x = rng.uniform(-5.0, 25.0, (rows, 3))
    x[NLOCAL:] = SENTINEL
    f = _exact_forces(rng, rows)
    f[NLOCAL + ng:] = SENTINEL
    shift = np.concatenate([rng.integers(-1, 2, (ng, 3)) * np.array([20.3, 17.9, 31.1]), np.full((TAIL, 3), SENTINEL)])
    return owner, x, f, shift


LAYOUTS = [(ng, "mixed") for ng in GHOSTS] + [(1500, "one")]


@pytest.mark.parametrize("ng,layout", LAYOUTS)
def test_forward_pack_and_append(ng, layout, dev):
    owner, x, f, shift = _ghost_case(ng, layout)
    to, ts = dev.up(owner), dev.up(shift)
    tx = dev.up(x)
    assert dev.lib.ani_md_forward_ghosts(tx.data_ptr(), to.data_ptr(), ts.data_ptr(), NLOCAL, ng, None) == 0
    _same(dev.down(tx)[0], mr.forward(x, owner, shift, NLOCAL), "forward")
    tx, out = dev.up(x), dev.up(np.full((ng + TAIL, 3), SENTINEL))
    assert dev.lib.ani_md_pack_ghosts(tx.data_ptr(), to.data_ptr(), ts.data_ptr(), ng, out.data_ptr(), None) == 0
    got_x, got = dev.down(tx, out)
    _same(got_x, x, "pack reads x only")
    _same(got, np.concatenate([mr.pack(x, owner, shift), np.full((TAIL, 3), SENTINEL)]), "pack")
    species = np.random.default_rng(ng).integers(0, 7, NLOCAL + ng + TAIL).astype(np.int32)
    species[NLOCAL:] = -9
    tx, tsp = dev.up(x), dev.up(species)
    assert dev.lib.ani_md_append_ghosts(tx.data_ptr(), tsp.data_ptr(), NLOCAL, to.data_ptr(), ts.data_ptr(), ng, None) == 0
    got_x, got_sp = dev.down(tx, tsp)
    xr, spr = mr.append(x, species, NLOCAL, owner, shift)
    _same(got_x, xr, "append x")
    _same(got_sp, spr, "append species")


@pytest.mark.parametrize("ng,layout", LAYOUTS)
def test_reverse_kernels_sum_exactly(ng, layout, dev):
    owner, x, f, shift = _ghost_case(ng, layout, seed=1)
    to = dev.up(owner)
    tf = dev.up(f)
    assert dev.lib.ani_md_reverse_ghosts(tf.data_ptr(), to.data_ptr(), NLOCAL, ng, None) == 0
    ref = mr.reverse(f, owner, NLOCAL)
    assert np.abs(ref[:NLOCAL]).max() < 2.0 ** 32                          # exact: multiples of 2^-20 below 2^32 fit 53 bits
    _same(dev.down(tf)[0], ref, "reverse")
    tf = dev.up(f)
    assert dev.lib.ani_md_reverse_ghosts_ordered(tf.data_ptr(), to.data_ptr(), None, NLOCAL, ng, None) == 0
    _same(dev.down(tf)[0], ref, "reverse_ordered without an order")
    ghost_of = np.random.default_rng(ng + 5).permutation(ng).astype(np.int64)
    tf, tg = dev.up(f), dev.up(ghost_of)
    assert dev.lib.ani_md_reverse_ghosts_ordered(tf.data_ptr(), to.data_ptr(), tg.data_ptr(), NLOCAL, ng, None) == 0
    _same(dev.down(tf)[0], mr.reverse_ordered(f, owner, ghost_of, NLOCAL), "reverse_ordered")
    inp = np.concatenate([_exact_forces(np.random.default_rng(ng + 6), ng), np.full((TAIL, 3), SENTINEL)])
    tf, ti = dev.up(f), dev.up(inp)
    assert dev.lib.ani_md_unpack_reverse(tf.data_ptr(), to.data_ptr(), ng, ti.data_ptr(), None) == 0
    got_f, got_in = dev.down(tf, ti)
    _same(got_f, mr.unpack_reverse(f, owner, inp), "unpack_reverse")
    _same(got_in, inp, "unpack_reverse reads its message only")


@pytest.mark.parametrize("n", GHOSTS)
def test_gather_and_scatter_rows(n, dev):
    rng = np.random.default_rng(n + 11)
    rows = n + 40
    src = rng.normal(0.0, 10.0, (rows, 3))
    idx = rng.permutation(rows)[:n].astype(np.int64)
    ts, ti, out = dev.up(src), dev.up(idx), dev.up(np.full((n + TAIL, 3), SENTINEL))
    assert dev.lib.ani_md_gather_rows(ts.data_ptr(), ti.data_ptr(), n, out.data_ptr(), None) == 0
    got_src, got = dev.down(ts, out)
    _same(got, np.concatenate([mr.gather(src, idx), np.full((TAIL, 3), SENTINEL)]), "gather")
    _same(got_src, src, "gather reads its source only")
    inp = np.concatenate([rng.normal(0.0, 10.0, (n, 3)), np.full((TAIL, 3), SENTINEL)])
    dst = np.full((rows, 3), SENTINEL)
    td, tin = dev.up(dst), dev.up(inp)
    assert dev.lib.ani_md_scatter_rows(td.data_ptr(), ti.data_ptr(), n, tin.data_ptr(), None) == 0
    _same(dev.down(td)[0], mr.scatter(dst, idx, inp), "scatter")
    if n:                                                                  # gather with repeated rows: every slot reads one owner
        rep = np.full(n, idx[0], dtype=np.int64)
        tr, out = dev.up(rep), dev.up(np.full((n + TAIL, 3), SENTINEL))
        assert dev.lib.ani_md_gather_rows(ts.data_ptr(), tr.data_ptr(), n, out.data_ptr(), None) == 0
        _same(dev.down(out)[0][:n], mr.gather(src, rep), "gather of one row")


# ---- wrap ------------------------------------------------------------------------------------------------------------------
# lo != 0 in every dimension; the boxes of the recorded counter-examples (4.4, 56.4) and (36.3, 34.8) sit in different dimensions
BOXES = (((4.4, 36.3, -12.7), (56.4, 34.8, 25.1)), ((36.3, -3.3, 4.4), (34.8, 17.9, 56.4)))
WRAP_ULPS = 4


@lru_cache(maxsize=None)
def _wrap_edges(lo, L):
    """exactly lo, lo + L, lo - L, lo + 2 L, four ulp-neighbours of each on both sides, and the recorded counter-examples"""
    out = [v for blo, bl, v in COUNTER_EXAMPLES if (blo, bl) == (lo, L)]
    for base in (lo + 2.0 * L, lo + L, lo - L, lo):
        out.append(base)
        for side in (-np.inf, np.inf):
            v = base
            for _ in range(4):
                v = float(np.nextafter(v, side))
                out.append(v)
    return tuple(out)


@lru_cache(maxsize=None)
def _wrap_truth(v, lo, L):
    """(t, bar) as Fractions.  With S = |v| + |lo| + L: the kernel rounds v - lo (one rounding of a value below S), the division
    (one more, relative), k L and the final subtraction (one each of values below S; a fused multiply-add saves one).  Where the
    integer k is the true one, out is off by the last two: 2 x 2^-53 S.  k can be off by one only where the first two moved the
    quotient across an integer, that is where t is within 2 x 2^-53 S of a face; the image then lands within that of the OTHER
    face: on or above lo + L, which the kernel sends to lo, or below lo, which is the clamp's case.  Bar: 4 x 2^-53 S."""
    t = mr.wrap_exact(v, lo, L)
    return t, Fraction(WRAP_ULPS) * Fraction(abs(v) + abs(lo) + L) / 2 ** 53


def _wrap_inputs(n, box, start):
    lo3, len3 = box
    rng = np.random.default_rng(n + start)
    x = np.empty((n, 3))
    for k in range(3):
        edges = _wrap_edges(lo3[k], len3[k])
        x[:, k] = lo3[k] + rng.uniform(-3.0, 4.0, n) * len3[k]                 # interior points up to 3 L away on either side
        m = min(n, len(edges))
        x[:m, k] = [edges[(start + 11 * k + i) % len(edges)] for i in range(m)]
    return x


@pytest.mark.parametrize("mask", range(8))
@pytest.mark.parametrize("n", [1, 85, 86, 1500])
def test_wrap_positions(n, mask, dev):
    outside, worst = [], 0.0
    for b, box in enumerate(BOXES):
        lo3, len3 = np.array(box[0]), np.array(box[1])
        starts = range(38) if n == 1 else (5 * mask + b,)                # a lone atom: walk through the edge values
        for start in starts:
            x = _wrap_inputs(n, box, start)
            tx = dev.up(x)
            assert dev.lib.ani_md_wrap_positions(tx.data_ptr(), n, lo3.ctypes.data, len3.ctypes.data, mask, None) == 0
            (out,) = dev.down(tx)
            for k in range(3):
                if not (mask >> k) & 1:
                    _same(out[:, k], x[:, k], f"non-periodic dimension {k}")
                    continue
                lo, L = float(lo3[k]), float(len3[k])
                flo, fhi = Fraction(lo), Fraction(lo) + Fraction(L)
                for i in range(n):
                    o, (t, bar) = Fraction(float(out[i, k])), _wrap_truth(float(x[i, k]), lo, L)
                    if not flo <= o < fhi:
                        outside.append((b, k, float(x[i, k]).hex(), float(out[i, k]).hex(), float(o - flo)))
                        continue
                    ok = abs(o - t) <= bar or (o == flo and fhi - t <= bar)
                    assert ok, (b, k, float(x[i, k]).hex(), float(out[i, k]).hex(), float(t), float(bar))
                    if abs(o - t) <= bar:
                        worst = max(worst, float(abs(o - t) / bar) * WRAP_ULPS)
    WORST["wrap"] = max(WORST.get("wrap", 0.0), worst)
    print(f"  n {n} mask {mask}: {len(outside)} coordinates outside [lo, lo + L); largest |out - t| {worst:.2f} x 2^-53 S "
          f"(bar {WRAP_ULPS}); worst so far {WORST['wrap']:.2f}")
    assert not outside, outside[:5]


# ---- ghost shell -----------------------------------------------------------------------------------------------------------
def _shell_case(n, ncombo, empty=False):
    """atoms on a grid of quarters in [0, 10), interval bounds on the same grid: atoms sit exactly ON faces.  ncombo >= 3: the
    first and the last combination are empty, combination 1 holds every atom, combination 2 has atom 0 exactly on its clo (in)
    and, from two atoms on, the last atom exactly on its chi in one dimension (out).  ncombo = 1: it holds every atom.
    empty: no combination has a hit."""
    rng = np.random.default_rng(1000 * ncombo + n)
    x = rng.integers(0, 40, (n, 3)) * 0.25
    clo = rng.integers(0, 30, (ncombo, 3)) * 0.25
    chi = clo + rng.integers(1, 20, (ncombo, 3)) * 0.25
    cshift = rng.integers(-1, 2, (ncombo, 3)) * np.array([10.0, 10.5, 11.25])
    if empty:
        clo += 100.0
        chi += 100.0
        return x, clo, chi, cshift
    hold_all = 0 if ncombo < 3 else 1
    clo[hold_all], chi[hold_all] = 0.0, 10.0
    if ncombo >= 3:
        clo[0], chi[0] = (10.0, 0.0, 0.0), (20.0, 10.0, 10.0)                   # starts where the atoms end
        clo[-1], chi[-1] = (0.0, 0.0, -5.0), (10.0, 10.0, 0.0)                  # ends where the atoms begin: x = 0 is ON its chi
        x[0] = (3.0, 4.25, 5.5)
        clo[2], chi[2] = x[0], x[0] + 2.5
        if n >= 2:
            x[n - 1] = (chi[2][0], clo[2][1], clo[2][2])
    return x, clo, chi, cshift


SHELL_CASES = [(n, c) for c in (1, 26, 124) for n in SIZES] + [(2048, 128), (2305, 124)]


@pytest.mark.parametrize("empty", [False, True], ids=["hits", "no_hit"])
@pytest.mark.parametrize("n,ncombo", SHELL_CASES)
def test_ghost_shell_count_scan_fill_append(n, ncombo, empty, dev):
    torch = dev.torch
    x, clo, chi, cshift = _shell_case(n, ncombo, empty)
    cnt, off, counts, idx, shift, ghosts = mr.shell(x, clo, chi, cshift)
    nblk, hits = max((n + 255) // 256, 1), len(idx)
    assert len(cnt) == ncombo * nblk
    if (n, ncombo) == (2048, 128):
        assert len(cnt) == 1024                                              # exactly one round of the scan
    if (n, ncombo) == (2305, 124) and not empty:
        assert len(cnt) == 1240 and cnt[:1024].sum() > 0 and cnt[1024:].sum() > 0   # two rounds, a carry, hits behind it
    if empty:
        assert hits == 0
    else:
        assert counts[1 + (0 if ncombo < 3 else 1)] == n
        if ncombo >= 3:
            assert counts[1] == 0 and counts[-1] == 0
            on_clo = (x[idx] == clo[np.repeat(np.arange(ncombo), counts[1:])]).any()
            assert on_clo and counts[3] >= 1 and (n < 2 or n - 1 not in idx[counts[1:3].sum():counts[1:4].sum()])
    tx, tlo, thi, tsh = dev.up(x), dev.up(clo), dev.up(chi), dev.up(cshift)
    fill = lambda k, dtype: torch.full((k,), -77, dtype=dtype, device=dev.dev)
    tcnt, toff, tcounts = fill(len(cnt) + TAIL, torch.int32), fill(len(cnt) + TAIL, torch.int32), fill(1 + ncombo + TAIL, torch.int32)
    assert dev.lib.ani_md_ghost_shell_count(tx.data_ptr(), n, tlo.data_ptr(), thi.data_ptr(), ncombo, tcnt.data_ptr(), toff.data_ptr(),
                                            tcounts.data_ptr(), None) == 0
    gcnt, goff, gcounts = dev.down(tcnt, toff, tcounts)
    tail = np.full(TAIL, -77, dtype=np.int32)
    _same(gcnt, np.concatenate([cnt, tail]), "blk_cnt")
    _same(goff, np.concatenate([off, tail]), "blk_off")
    _same(gcounts, np.concatenate([counts, tail]), "out_counts")
    assert gcounts[0] == hits
    tidx = fill(hits + TAIL, torch.int64)
    tshift = dev.up(np.full((hits + TAIL, 3), SENTINEL))
    assert dev.lib.ani_md_ghost_shell_fill(tx.data_ptr(), n, tlo.data_ptr(), thi.data_ptr(), tsh.data_ptr(), ncombo, toff.data_ptr(),
                                           tidx.data_ptr(), tshift.data_ptr(), None) == 0
    gidx, gshift = dev.down(tidx, tshift)
    _same(gidx, np.concatenate([idx, np.full(TAIL, -77, dtype=np.int64)]), "send_idx")
    _same(gshift, np.concatenate([shift.reshape(-1, 3), np.full((TAIL, 3), SENTINEL)]), "send_shift")
    # the ghosts themselves, appended behind the owned block from the device's own lists
    xa = np.concatenate([x, np.full((hits + TAIL, 3), SENTINEL)])
    species = np.concatenate([np.random.default_rng(n).integers(0, 7, n), np.full(hits + TAIL, -9)]).astype(np.int32)
    txa, tsp = dev.up(xa), dev.up(species)
    assert dev.lib.ani_md_append_ghosts(txa.data_ptr(), tsp.data_ptr(), n, tidx.data_ptr(), tshift.data_ptr(), hits, None) == 0
    gx, gsp = dev.down(txa, tsp)
    _same(gx, np.concatenate([x, ghosts.reshape(-1, 3), np.full((TAIL, 3), SENTINEL)]), "appended ghosts")
    _same(gsp, mr.append(xa, species, n, idx, shift.reshape(-1, 3))[1], "appended species")


# ---- check -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [-1234.5, 0.0, float("nan"), float("inf"), -float("inf")], ids=repr)
def test_check_returns_the_maximum_or_infinity_and_zeroes_it(e, dev):
    d2 = float(np.nextafter(2.5, 3.0))
    td, tev, out = dev.up(np.array([d2, SENTINEL])), dev.up(np.array([e, 1.0, 2.0])), dev.up(np.array([SENTINEL, SENTINEL]))
    assert dev.lib.ani_md_check(td.data_ptr(), tev.data_ptr(), out.data_ptr(), None) == 0
    gd, gev, gout = dev.down(td, tev, out)
    want, after = mr.check(d2, e)
    _same(gout, np.array([want, SENTINEL]), "out")
    _same(gd, np.array([after, SENTINEL]), "d2max")
    assert gev.tobytes() == np.array([e, 1.0, 2.0]).tobytes()
