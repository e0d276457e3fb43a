"""GPU: the Nose-Hoover chain kernels and the thermo record of include/ani_md.h (ani_md_nh_*, ani_md_thermo), one call at a time
through ctypes, against the numpy forms of tests/nh_reference.py.

Sums.  Every term of K2 and of the diagonal sums is positive, so any order of summation of n terms stays within (n - 1) 2^-53
relative of the exact sum, and the few roundings inside a term (on either side) within a few 2^-53 more: the bar is
(n + 16) 2^-52 of the sum (of the sum of the magnitudes for the off-diagonal sums, whose terms have either sign).
Chain.  The bars are nh_reference.chain_bars: ten times the reference's own rounding (tests/test_nh_reference_cpu.py holds the
reference to a tenth of them on the same cases).
Integrators.  The bars of tests/test_md_loop_kernels.py (its module docstring: |device - reference| <= (2 c + 1) 2^-53 M for c
roundings in the unfused chain), with one rounding more for s v:  v' = s v + dtfm f has c = 3, M = |s v| + dtfm |f|;
x' = x + dt v' has c = 5;  the final kick is the unsuffixed kernel's, c = 2.  ani_md_nh_scale is a single multiplication: bit
for bit.
"""
import math

import numpy as np
import pytest

import nh_reference as nh
from test_md_loop_kernels import Device, _d2_bar, _same, _within

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 513, 65537]          # the last: 257 partials, more than the 256 threads of the finishing workgroup
U2 = 2.0 ** -52
DT = 0.5


@pytest.fixture(scope="module")
def dev():
    from lammps_ani_amd import ani_hip
    return Device(ani_hip)


def _atoms(n, seed=0):
    rng = np.random.default_rng(5000 + 17 * seed + n)
    mass = nh.MASSES[rng.integers(0, 7, n)]
    v = rng.normal(0.0, 0.01, (n, 3)) * rng.choice([0.1, 1.0, 3.0], (n, 1))
    return mass, v, rng


def _blocks(a, n):
    return [a[b:b + 256] for b in range(0, n, 256)]


def _params(ani_hip, c):
    return ani_hip.NhParams(c["dt"], c["t_period"], c["drag"], c["M"], c["nc"])


# ---- sums ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_k2_partials_and_tensor_sums_against_fsum(n, dev):
    lib, torch = dev.lib, dev.torch
    mass, v, _ = _atoms(n)
    nblk = (n + 255) // 256
    assert lib.ani_md_nh_work_size(n) == nblk and lib.ani_md_thermo_work_size(n) == 6 * nblk
    tv, tm = dev.up(v), dev.up(mass)
    parts = []
    for _ in range(2):
        w = torch.full((nblk + 3,), -7777.25, dtype=torch.float64, device=dev.dev)
        assert lib.ani_md_nh_kinetic(tv.data_ptr(), tm.data_ptr(), n, w.data_ptr(), None) == 0
        parts.append(dev.down(w)[0])
    _same(parts[0], parts[1], "two launches of ani_md_nh_kinetic")
    assert (parts[0][nblk:] == -7777.25).all()
    p = parts[0][:nblk]
    for b, (mb, vb) in enumerate(zip(_blocks(mass, n), _blocks(v, n))):
        ref = nh.k2_sum(vb, mb)
        assert abs(p[b] - ref) <= (len(mb) + 16) * U2 * ref, (b, p[b], ref)
    k2 = nh.k2_sum(v, mass)
    got = math.fsum(p.tolist())
    print(f"  n {n}: K2 {got!r} against {k2!r}, off by {abs(got - k2) / k2 / U2:.2f} x 2^-52 (bar {n + 16})")
    assert abs(got - k2) <= (n + 16) * U2 * k2
    # the six sums and K2 through both launches of ani_md_thermo
    K, mag = nh.tensor_sums(v, mass)
    tev = dev.up(np.zeros(10))
    outs = []
    for _ in range(2):
        work = torch.full((6 * nblk + 3,), -7777.25, dtype=torch.float64, device=dev.dev)
        out = torch.full((nh.THERMO_N + 3,), -7777.25, dtype=torch.float64, device=dev.dev)
        assert lib.ani_md_thermo(tv.data_ptr(), tm.data_ptr(), n, tev.data_ptr(), 1, 3.0 * n, 1.0, None, work.data_ptr(),
                                 out.data_ptr(), None) == 0
        w, o = dev.down(work, out)
        assert (w[6 * nblk:] == -7777.25).all() and (o[nh.THERMO_N:] == -7777.25).all()
        outs.append((w, o))
    _same(outs[0][0], outs[1][0], "two launches of ani_md_thermo, partials")
    _same(outs[0][1], outs[1][1], "two launches of ani_md_thermo, record")
    o = outs[0][1]
    # volume 1 and no virial: out[4 + c] = K_c nktv2p, one more rounding
    for c in range(6):
        assert abs(o[4 + c] / nh.NKTV2P - K[c]) <= (n + 16) * U2 * mag[c] + 2 * U2 * abs(K[c]), (c, o[4 + c] / nh.NKTV2P, K[c])
    tr = K[0] + K[1] + K[2]
    assert abs(o[14] - tr) <= (n + 16) * U2 * tr and abs(o[14] - k2) <= 2 * (n + 16) * U2 * k2 and o[1] == 0.5 * o[14]


def test_chain_sums_more_partials_than_it_has_threads(dev):
    """257 and 600 partials whose every partial sum is exact (multiples of 2^-10 below 2^20): the chain's record from the partials
    is bit for bit the record from their sum in state[1], which it could not be with a partial left out or taken twice"""
    from lammps_ani_amd import ani_hip
    lib = dev.lib
    c = nh.chain_cases()[0]
    par = _params(ani_hip, c)
    for npart in (1, 2, 255, 256, 257, 600):
        rng = np.random.default_rng(npart)
        w = rng.integers(1, 1 << 20, npart).astype(np.float64) * 2.0 ** -10
        w[-1] += 2.0 ** 12                                               # the last one counts visibly
        total = float(w.sum())
        assert total == math.fsum(w.tolist())
        rec = nh.state_record(4, 123.0, 0.5, 1.0, 2.0, 3.0, 0, c["eta"], c["eta_dot"], c["eta_dotdot"])
        a, b, tw = dev.up(rec), dev.up(rec), dev.up(w)
        b[1] = total
        assert lib.ani_md_nh_chain(a.data_ptr(), tw.data_ptr(), npart, c["t_target"], c["tdof"], par, None) == 0
        assert lib.ani_md_nh_chain(b.data_ptr(), None, 0, c["t_target"], c["tdof"], par, None) == 0
        ra, rb = dev.down(a, b)
        _same(ra, rb, f"record from {npart} partials against the record from their sum")
        ref = nh.chain_half_step(total, c["t_target"], c["tdof"], c["dt"], c["t_period"], c["drag"], c["M"], c["nc"], c["eta"],
                                 c["eta_dot"], c["eta_dotdot"])
        assert abs(ra[1] - ref["K2"]) <= 1e-14 * ref["K2"] and ra[0] == 5.0


# ---- chain -----------------------------------------------------------------------------------------------------------------
def test_chain_half_step_on_the_drawn_cases(dev):
    from lammps_ani_amd import ani_hip
    lib, torch = dev.lib, dev.torch
    cases = nh.chain_cases()
    nc = len(cases)
    recs = np.stack([nh.state_record(7, -1.0, -2.0, -3.0, -4.0, -5.0, 2, c["eta"], c["eta_dot"], c["eta_dotdot"]) for c in cases])
    from_state = recs.copy()
    from_state[:, 1] = [c["K2"] for c in cases]
    ta, tb, tw = dev.up(recs), dev.up(from_state), dev.up(np.array([c["K2"] for c in cases]))
    for i, c in enumerate(cases):
        par = _params(ani_hip, c)
        assert lib.ani_md_nh_chain(ta[i].data_ptr(), tw[i:].data_ptr(), 1, c["t_target"], c["tdof"], par, None) == 0
        assert lib.ani_md_nh_chain(tb[i].data_ptr(), None, 0, c["t_target"], c["tdof"], par, None) == 0
    ga, gb = dev.down(ta, tb)
    _same(ga, gb, "npart > 0 against npart == 0 for the same K2")
    worst = dict(eta=0.0, eta_dot=0.0, eta_dotdot=0.0, s=0.0, K2=0.0, ecouple=0.0)
    for i, c in enumerate(cases):
        M, g = c["M"], ga[i]
        r = nh.chain_half_step(c["K2"], c["t_target"], c["tdof"], c["dt"], c["t_period"], c["drag"], M, c["nc"], c["eta"],
                               c["eta_dot"], c["eta_dotdot"])
        bars = nh.chain_bars(c, r)
        got = dict(eta=g[8:8 + M], eta_dot=g[16:16 + M], eta_dotdot=g[24:24 + M], s=g[2], K2=g[1], ecouple=g[4])
        for key in worst:
            err = np.abs(got[key] - np.asarray(r[key], dtype=np.float64))
            worst[key] = max(worst[key], float(np.max(err / bars[key])))
            assert (err <= bars[key]).all(), (i, key, got[key], r[key], bars[key])
        assert g[0] == 8.0 and g[3] == c["t_target"] and g[5] == c["tdof"] and g[6] == 2.0 and g[7] == 0.0
        for k in range(3):
            assert (g[8 + 8 * k + M: 16 + 8 * k] == 0.0).all()           # unused links stay 0
    print("  largest |device - reference| as a fraction of the bar:", {k: f"{w:.3f}" for k, w in worst.items()})


def test_chain_on_target_at_rest_and_with_a_non_finite_sum(dev):
    from lammps_ani_amd import ani_hip
    lib = dev.lib
    for M in (1, 3, 8):
        tdof, T = 87.0, 300.0
        par = ani_hip.NhParams(0.5, 50.0, 0.0, M, 2)
        ket = float(nh.chain_masses(T, tdof, 50.0, M)[1])
        st, tw = dev.up(np.zeros(nh.NSTATE)), dev.up(np.array([ket]))
        assert lib.ani_md_nh_chain(st.data_ptr(), tw.data_ptr(), 1, T, tdof, par, None) == 0
        (g,) = dev.down(st)
        assert g[2] == 1.0 and g[1] == ket and g[8] == 0.0 and g[16] == 0.0 and g[24] == 0.0 and g[0] == 1.0
    c = nh.chain_cases()[3]
    par = _params(ani_hip, c)
    rec = nh.state_record(7, 55.0, 0.9, 1.0, -4.0, 5.0, 0, c["eta"], c["eta_dot"], c["eta_dotdot"])
    for bad in (float("nan"), float("inf")):
        for npart in (1, 0):
            start = rec.copy()
            if npart == 0:
                start[1] = bad
            st, tw = dev.up(start), dev.up(np.array([bad]))
            assert lib.ani_md_nh_chain(st.data_ptr(), tw.data_ptr(), npart, c["t_target"], c["tdof"], par, None) == 0
            (g,) = dev.down(st)
            assert g[2] == 1.0 and g[6] == 1.0 and g[0] == 7.0 and g[4] == -4.0 and not np.isfinite(g[1])
            _same(g[8:], rec[8:], "the chain after a non-finite K2")
    # parameters that cannot be: refused on the host, nothing launched
    st = dev.up(rec)
    for args in ((0.5, 50.0, 0.0, 0, 1), (0.5, 50.0, 0.0, 9, 1), (0.5, 50.0, 0.0, 3, 0), (0.5, 0.0, 0.0, 3, 1)):
        assert lib.ani_md_nh_chain(st.data_ptr(), None, 0, 300.0, 87.0, ani_hip.NhParams(*args), None) != 0
    assert lib.ani_md_nh_chain(st.data_ptr(), None, 0, 0.0, 87.0, par, None) != 0
    _same(dev.down(st)[0], rec, "a refused call writes nothing")
    assert lib.ani_md_nh_init(st.data_ptr(), None) == 0
    _same(dev.down(st)[0], np.zeros(nh.NSTATE), "ani_md_nh_init")


# ---- scale and the scaled integrators ----------------------------------------------------------------------------------------
def _integrator_inputs(n, seed):
    mass, v, rng = _atoms(n, seed)
    p = dict(x=rng.uniform(0.0, 20.0, (n, 3)), v=v, f=rng.normal(0.0, 15.0, (n, 3)), mass=mass, s=(0.5 * DT * nh.FTM2V) / mass)
    p["xb"] = p["x"] + rng.normal(0.0, 0.05, (n, 3))
    return p


def _state_with_s(s):
    rec = np.zeros(nh.NSTATE)
    rec[2] = s
    return rec


@pytest.mark.parametrize("n", SIZES)
def test_scale_and_initial_integrate(n, dev):
    lib = dev.lib
    p = _integrator_inputs(n, 1)
    sc = 0.99873046875 + 1e-9
    st = dev.up(_state_with_s(sc))
    tv = dev.up(np.concatenate([p["v"], np.full((2, 3), -7777.25)]))
    assert lib.ani_md_nh_scale(tv.data_ptr(), n, st.data_ptr(), None) == 0
    _same(dev.down(tv)[0], np.concatenate([nh.scale(p["v"], sc), np.full((2, 3), -7777.25)]), "ani_md_nh_scale")
    tx, tv, tf, ts, txb = (dev.up(p[k]) for k in ("x", "v", "f", "s", "xb"))
    d = dev.up(np.array([0.0]))
    assert lib.ani_md_nh_initial_integrate(tx.data_ptr(), tv.data_ptr(), tf.data_ptr(), ts.data_ptr(), DT, n, txb.data_ptr(), d.data_ptr(),
                                           st.data_ptr(), None) == 0
    x, v, f, d = dev.down(tx, tv, tf, d)
    xr, vr, dr = nh.nh_initial_integrate(p["x"], p["v"], p["f"], p["s"], DT, p["xb"], 0.0, sc)
    mv = np.abs(sc * p["v"]) + p["s"][:, None] * np.abs(p["f"])
    mx = np.abs(p["x"]) + DT * mv
    _within(v, vr, 3, mv, "nh_initial_integrate v")
    _within(x, xr, 5, mx, "nh_initial_integrate x")
    _same(f, p["f"], "f is read only")
    bar = _d2_bar(xr, p["xb"], 5, mx)
    print(f"  d2max {d[0]!r} against {dr!r}: off by {abs(d[0] - dr):.3e}, bar {bar:.3e}")
    assert abs(d[0] - dr) <= bar
    # a running maximum above every displacement stays as it is; s = 1 is the unsuffixed kernel bit for bit
    tx, tv, d1 = dev.up(p["x"]), dev.up(p["v"]), dev.up(np.array([1.0e3]))
    one = dev.up(_state_with_s(1.0))
    assert lib.ani_md_nh_initial_integrate(tx.data_ptr(), tv.data_ptr(), tf.data_ptr(), ts.data_ptr(), DT, n, txb.data_ptr(), d1.data_ptr(),
                                           one.data_ptr(), None) == 0
    ux, uv, d0 = dev.up(p["x"]), dev.up(p["v"]), dev.up(np.array([0.0]))
    assert lib.ani_md_initial_integrate(ux.data_ptr(), uv.data_ptr(), tf.data_ptr(), ts.data_ptr(), DT, n, txb.data_ptr(), d0.data_ptr(),
                                        None) == 0
    x1, v1, d1, x0, v0 = dev.down(tx, tv, d1, ux, uv)
    assert d1[0] == 1.0e3
    _same(x1, x0, "x with s = 1 against ani_md_initial_integrate")
    _same(v1, v0, "v with s = 1 against ani_md_initial_integrate")


@pytest.mark.parametrize("n", SIZES)
def test_final_integrate_and_its_partials(n, dev):
    lib, torch = dev.lib, dev.torch
    p = _integrator_inputs(n, 2)
    nblk = (n + 255) // 256
    rows = n + 2                                                           # two rows behind nlocal, which nothing may touch
    vin = np.concatenate([p["v"], np.full((2, 3), -7777.25)])
    tv, tf, ts, tm = dev.up(vin), dev.up(p["f"]), dev.up(p["s"]), dev.up(p["mass"])
    w = torch.full((nblk + 3,), -7777.25, dtype=torch.float64, device=dev.dev)
    assert lib.ani_md_nh_final_integrate(tv.data_ptr(), tf.data_ptr(), ts.data_ptr(), tm.data_ptr(), n, w.data_ptr(), None) == 0
    v, f, part = dev.down(tv, tf, w)
    vr, k2 = nh.nh_final_integrate(p["v"], p["f"], p["s"], p["mass"])
    _within(v[:n], vr, 2, np.abs(p["v"]) + p["s"][:, None] * np.abs(p["f"]), "nh_final_integrate v")
    _same(v[n:], vin[n:], "rows behind nlocal")
    _same(f, p["f"], "f is read only")
    assert rows == len(v) and (part[nblk:] == -7777.25).all()
    # against the unsuffixed kernel: the same velocities bit for bit
    uv = dev.up(p["v"])
    assert lib.ani_md_final_integrate(uv.data_ptr(), tf.data_ptr(), ts.data_ptr(), n, 0, None, None, None, 0, 0, None) == 0
    _same(v[:n], dev.down(uv)[0], "v against ani_md_final_integrate")
    # the partials are those of ani_md_nh_kinetic on the velocities it wrote, bit for bit, and their sum is the new K2
    w2 = torch.full((nblk + 3,), -7777.25, dtype=torch.float64, device=dev.dev)
    assert lib.ani_md_nh_kinetic(tv.data_ptr(), tm.data_ptr(), n, w2.data_ptr(), None) == 0
    _same(part, dev.down(w2)[0], "partials of ani_md_nh_final_integrate against ani_md_nh_kinetic on its output")
    got, ref = math.fsum(part[:nblk].tolist()), nh.k2_sum(v[:n], p["mass"])
    assert abs(got - ref) <= (n + 16) * U2 * ref


def test_no_owned_atoms_touch_nothing(dev):
    lib = dev.lib
    p = _integrator_inputs(4, 3)
    st = dev.up(_state_with_s(0.5))
    tx, tv, tf, ts, txb, tm = (dev.up(p[k]) for k in ("x", "v", "f", "s", "xb", "mass"))
    d, w = dev.up(np.array([3.5])), dev.up(np.array([-7777.25]))
    assert lib.ani_md_nh_initial_integrate(tx.data_ptr(), tv.data_ptr(), tf.data_ptr(), ts.data_ptr(), DT, 0, txb.data_ptr(), d.data_ptr(),
                                           st.data_ptr(), None) == 0
    assert lib.ani_md_nh_final_integrate(tv.data_ptr(), tf.data_ptr(), ts.data_ptr(), tm.data_ptr(), 0, w.data_ptr(), None) == 0
    assert lib.ani_md_nh_scale(tv.data_ptr(), 0, st.data_ptr(), None) == 0
    assert lib.ani_md_nh_kinetic(tv.data_ptr(), tm.data_ptr(), 0, w.data_ptr(), None) == 0
    x, v, d, w = dev.down(tx, tv, d, w)
    _same(x, p["x"], "x"), _same(v, p["v"], "v")
    assert d[0] == 3.5 and w[0] == -7777.25


# ---- thermo ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 1500])
def test_thermo_record(n, dev):
    lib, torch = dev.lib, dev.torch
    mass, v, rng = _atoms(n, 4)
    ev = np.concatenate([[-1234.5 * n], rng.normal(0.0, 40.0, 9) * n])
    tdof, vol, ec = 3.0 * n - 3.0 + 3.0 * (n == 1), 9.3 ** 3 * n, -3.25
    st = dev.up(nh.state_record(9, 1.0, 1.0, 300.0, ec, tdof, 0, [0.1], [0.2], [0.3]))
    tv, tm, tev = dev.up(v), dev.up(mass), dev.up(ev)
    work = torch.empty(lib.ani_md_thermo_work_size(n), dtype=torch.float64, device=dev.dev)
    K, mag = nh.tensor_sums(v, mass)
    for with_virial in (1, 0):
        for state in (st, None):
            out = torch.full((nh.THERMO_N,), -7777.25, dtype=torch.float64, device=dev.dev)
            assert lib.ani_md_thermo(tv.data_ptr(), tm.data_ptr(), n, tev.data_ptr(), with_virial, tdof, vol,
                                     None if state is None else state.data_ptr(), work.data_ptr(), out.data_ptr(), None) == 0
            (o,) = dev.down(out)
            e = ec if state is not None else 0.0
            r = nh.thermo(v, mass, ev, with_virial, tdof, vol, e)
            sum_bar = (n + 16) * U2
            k2_bar = sum_bar * r[14]
            assert o[0] == ev[0] and o[13] == vol and o[15] == 0.0 and o[11] == e
            assert abs(o[14] - r[14]) <= k2_bar and abs(o[1] - r[1]) <= 0.5 * k2_bar and abs(o[2] - r[2]) <= (sum_bar + 4 * U2) * r[2]
            assert abs(o[10] - r[10]) <= 0.5 * k2_bar + 2 * U2 * (abs(ev[0]) + r[1])
            assert abs(o[12] - r[12]) <= 0.5 * k2_bar + 4 * U2 * (abs(ev[0]) + r[1] + abs(e))
            if not with_virial:
                assert np.isnan(o[3:10]).all() and np.isfinite(np.delete(o, range(3, 10))).all()
                continue
            scale = nh.NKTV2P / vol
            wtr = abs(ev[1]) + abs(ev[5]) + abs(ev[9])
            assert abs(o[3] - r[3]) <= (k2_bar + 6 * U2 * (r[14] + wtr)) * scale / 3.0, (o[3], r[3])
            for c in range(6):
                wc = abs(ev[nh.W_INDEX[c]])
                assert abs(o[4 + c] - r[4 + c]) <= (sum_bar * mag[c] + 6 * U2 * (abs(K[c]) + wc)) * scale, (c, o[4 + c], r[4 + c])
            assert nh.W_INDEX == (1, 5, 9, 2, 3, 6)
            # the formula of the record, spelled out once more from the record's own entries
            assert np.isclose(o[3], (o[4] + o[5] + o[6]) / 3.0, rtol=1e-12)
