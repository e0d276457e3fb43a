"""GPU: the barostat kernels of include/ani_md.h (ani_md_npt_*), one call at a time through ctypes, against the numpy forms of
tests/npt_reference.py.

Chain.  ani_md_npt_chain in both phases on the drawn records of npt_reference.npt_cases, one launch each; bars per record entry
from npt_reference.half_step_bars: ten times the reference's own rounding (float64 against np.longdouble on that case), floored as
nh_reference.chain_bars floors the chain's outputs (tests/test_npt_reference_cpu.py holds the float64 reference to a tenth of them).
Integrators.  The bars of tests/test_md_loop_kernels.py (|device - reference| <= (2 c + 1) 2^-53 M for c roundings in the unfused
chain):  v' = (s fv) v + dtfm f has c = 4 (s fv, its product with v, dtfm f, the sum), M = |s fv v| + dtfm |f|;
x' = c + mu ((c + mu (x - c) + dt v') - c) has, on top of c(v') = 4: x - c, mu ., c + ., dt v', + ., - c, mu ., c + . = 8 more,
c = 12, M = 2 |c| + |x| + |x - c| + dt M(v') (mu is within a few per cent of 1: M carries a factor mu^2 for it);  the final kick
(v + dtfm f) fv has c = 3.  The shift rows are one multiplication: bit for bit.
"""
import math

import numpy as np
import pytest

import nh_reference as nh
import npt_reference as nr
from test_md_loop_kernels import Device, SENTINEL, _d2_bar, _same, _within

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1000]
GHOSTS = [0, 1, 300]
DT = 0.5


@pytest.fixture(scope="module")
def dev():
    from lammps_ani_amd import ani_hip
    return Device(ani_hip)


def _params(ani_hip, c):
    return ani_hip.NptParams(c["dt"], c["t_period"], c["drag"], c["p_period"], c["M"], c["nc"], c["Mp"], c["ncp"])


def _ev(wtr):
    """a virial whose trace is wtr exactly as the kernel sums it: (ev[1] + ev[5]) + ev[9]; the off-diagonal entries are noise"""
    ev = np.full(10, 123.456)
    ev[0], ev[1], ev[5], ev[9] = -50.0, wtr, 0.0, 0.0
    return ev


def _chain_call(dev, phase, c, ns, ps, from_partials=True, wtr=None, K2=None):
    from lammps_ani_amd import ani_hip
    ns = np.array(ns)
    K2 = c["K2"] if K2 is None else K2
    if not from_partials:
        ns[1] = K2
    tn, tp, tw, tev = dev.up(ns), dev.up(ps), dev.up(np.array([K2])), dev.up(_ev(c["wtr"] if wtr is None else wtr))
    rc = dev.lib.ani_md_npt_chain(phase, tn.data_ptr(), tp.data_ptr(), tw.data_ptr() if from_partials else None, 1 if from_partials else 0,
                                  tev.data_ptr(), c["t_target"], c["p_target"], c["tdof"], _params(ani_hip, c), None)
    assert rc == 0
    return dev.down(tn, tp)


@pytest.mark.parametrize("phase", [0, 1])
def test_chain_on_the_drawn_records(phase, dev):
    from lammps_ani_amd import ani_hip
    lib = dev.lib
    cases = nr.npt_cases()
    tn = dev.up(np.stack([c["ns"] for c in cases]))
    tp = dev.up(np.stack([c["ps"] for c in cases]))
    tn2, tp2 = tn.clone(), tp.clone()
    tw = dev.up(np.array([c["K2"] for c in cases]))
    tev = dev.up(np.stack([_ev(c["wtr"]) for c in cases]))
    for i, c in enumerate(cases):
        par = _params(ani_hip, c)
        for a, b in ((tn, tp), (tn2, tp2)):                               # twice on the same inputs
            assert lib.ani_md_npt_chain(phase, a[i].data_ptr(), b[i].data_ptr(), tw[i:].data_ptr(), 1, tev[i].data_ptr(), c["t_target"],
                                        c["p_target"], c["tdof"], par, None) == 0
    gn, gp, gn2, gp2 = dev.down(tn, tp, tn2, tp2)
    _same(gn, gn2, "two launches, NH record")
    _same(gp, gp2, "two launches, barostat record")
    worst_n, worst_p = np.zeros(nh.NSTATE), np.zeros(nr.NSTATE)
    for i, c in enumerate(cases):
        ns, ps, bn, bp = nr.half_step_bars(phase, c)
        for got, ref, bar, worst, what in ((gn[i], ns, bn, worst_n, "NH"), (gp[i], ps, bp, worst_p, "barostat")):
            err = np.abs(got - ref)
            nz = bar > 0.0
            worst[nz] = np.maximum(worst[nz], err[nz] / bar[nz])
            assert (err <= bar).all(), (i, what, np.flatnonzero(err > bar).tolist(), got[err > bar], ref[err > bar], bar[err > bar])
        assert gn[i][0] == 8.0 and gn[i][3] == c["t_target"] and gn[i][6] == 2.0 and gp[i][nr.PS_COUNT] == 7.0
        assert gp[i][nr.PS_PTARGET] == c["p_target"] and gp[i][nr.PS_NONFINITE] == 1.0 and gp[i][nr.PS_NATOMS] == c["N"]
        if phase == 1:                                                    # the second half leaves box, fv, mu, ratio and omega alone
            keep = [nr.PS_OMEGA, nr.PS_FV, nr.PS_MU] + list(range(nr.PS_LO, nr.PS_C))
            _same(gp[i][keep], c["ps"][keep], "what phase 1 does not write")
        _same(gp[i][nr.PS_C:nr.PS_V0 + 1], c["ps"][nr.PS_C:nr.PS_V0 + 1], "c and V0")
    print(f"  phase {phase}: largest |device - reference| / bar: NH record {worst_n.max():.3f} (entry {int(worst_n.argmax())}), "
          f"barostat record {worst_p.max():.3f} (entry {int(worst_p.argmax())})")


def test_chain_from_the_partials_and_from_the_record(dev):
    """npart > 0 sums the partials in the fixed order of ani_md_nh_chain: 600 partials whose every partial sum is exact give bit for
    bit the record that their sum in nh_state[1] gives"""
    from lammps_ani_amd import ani_hip
    c = nr.npt_cases()[1]
    for phase in (0, 1):
        for npart in (1, 257, 600):
            rng = np.random.default_rng(npart)
            w = rng.integers(1, 1 << 20, npart).astype(np.float64) * 2.0 ** -10
            total = float(w.sum())
            assert total == math.fsum(w.tolist())
            ns2 = c["ns"].copy()
            ns2[1] = total
            tn, tp, tn2, tp2, tw, tev = (dev.up(a) for a in (c["ns"], c["ps"], ns2, c["ps"], w, _ev(c["wtr"])))
            par = _params(ani_hip, c)
            assert dev.lib.ani_md_npt_chain(phase, tn.data_ptr(), tp.data_ptr(), tw.data_ptr(), npart, tev.data_ptr(), c["t_target"],
                                            c["p_target"], c["tdof"], par, None) == 0
            assert dev.lib.ani_md_npt_chain(phase, tn2.data_ptr(), tp2.data_ptr(), None, 0, tev.data_ptr(), c["t_target"],
                                            c["p_target"], c["tdof"], par, None) == 0
            a, b, a2, b2 = dev.down(tn, tp, tn2, tp2)
            _same(a, a2, "NH record from partials against from the record")
            _same(b, b2, "barostat record from partials against from the record")


def test_non_finite_half_step_and_refused_parameters(dev):
    from lammps_ani_amd import ani_hip
    c = nr.npt_cases()[2]
    keep = [nr.PS_COUNT, nr.PS_WD, nr.PS_OMEGA, nr.PS_P, nr.PS_W] + list(range(nr.PS_LO, nr.PS_RATIO)) + \
        list(range(nr.PS_C, nr.PS_NONFINITE)) + list(range(nr.PS_NATOMS, nr.NSTATE))
    for phase in (0, 1):
        for what, kw in (("K2 nan", dict(K2=float("nan"))), ("K2 inf", dict(K2=float("inf"), from_partials=False)),
                         ("Wtr inf", dict(wtr=float("inf"))), ("Wtr nan", dict(wtr=float("nan")))):
            gn, gp = _chain_call(dev, phase, c, c["ns"], c["ps"], **kw)
            assert gn[2] == 1.0 and gp[nr.PS_FV] == 1.0 and gp[nr.PS_MU] == 1.0 and (gp[nr.PS_RATIO:nr.PS_RATIO + 3] == 1.0).all(), what
            assert gn[6] == 3.0 and gp[nr.PS_NONFINITE] == 2.0 and gn[0] == 7.0 and gn[4] == -4.0, what
            _same(gp[keep], c["ps"][keep], f"{what}: box, strain rate and barostat chain")
            _same(gn[8:], c["ns"][8:], f"{what}: thermostat chain")
    # a strain rate that overflows in the update: K2 and Wtr finite, the new wd not
    ps = c["ps"].copy()
    ps[nr.PS_WD] = 1e308
    gn, gp = _chain_call(dev, 0, c, c["ns"], ps)
    assert gp[nr.PS_NONFINITE] == 2.0 and gp[nr.PS_WD] == 1e308 and gn[2] == 1.0 and gp[nr.PS_MU] == 1.0
    _same(gp[nr.PS_LO:nr.PS_RATIO], ps[nr.PS_LO:nr.PS_RATIO], "box after an overflowing strain rate")
    # parameters that cannot be: refused on the host, nothing launched
    tn, tp, tev = dev.up(c["ns"]), dev.up(c["ps"]), dev.up(_ev(1.0))
    good = (c["dt"], c["t_period"], c["drag"], c["p_period"], c["M"], c["nc"], c["Mp"], c["ncp"])
    for k, bad in ((3, 0.0), (6, 0), (6, 9), (7, 0), (4, 9), (1, -1.0)):
        args = list(good)
        args[k] = bad
        assert dev.lib.ani_md_npt_chain(0, tn.data_ptr(), tp.data_ptr(), None, 0, tev.data_ptr(), 300.0, 1.0, 87.0, ani_hip.NptParams(*args),
                                        None) != 0
    par = ani_hip.NptParams(*good)
    assert dev.lib.ani_md_npt_chain(2, tn.data_ptr(), tp.data_ptr(), None, 0, tev.data_ptr(), 300.0, 1.0, 87.0, par, None) != 0
    assert dev.lib.ani_md_npt_chain(0, tn.data_ptr(), tp.data_ptr(), None, 0, tev.data_ptr(), 300.0, float("nan"), 87.0, par, None) != 0
    gn, gp = dev.down(tn, tp)
    _same(gn, c["ns"], "a refused call writes nothing"), _same(gp, c["ps"], "a refused call writes nothing")


def test_init_and_check(dev):
    lib = dev.lib
    lo, length = np.array([-4.0, 1.5, 0.25]), np.array([8.0, 9.5, 7.75])
    tp = dev.up(np.full(nr.NSTATE + 2, SENTINEL))
    assert lib.ani_md_npt_init(tp.data_ptr(), lo.ctypes.data, length.ctypes.data, 30, None) == 0
    (g,) = dev.down(tp)
    _same(g[:nr.NSTATE], nr.init_record(lo, length, 30), "ani_md_npt_init")
    assert (g[nr.NSTATE:] == SENTINEL).all()
    bad = length.copy()
    bad[1] = 0.0
    assert lib.ani_md_npt_init(tp.data_ptr(), lo.ctypes.data, bad.ctypes.data, 30, None) != 0
    assert lib.ani_md_npt_init(tp.data_ptr(), lo.ctypes.data, length.ctypes.data, 0, None) != 0
    # the check: the word, then the record behind it; the word is zeroed; a non-finite energy turns the word into +inf
    rec = nr.npt_cases()[0]["ps"]
    for e, want in ((-12.5, 0.75), (float("nan"), float("inf")), (float("inf"), float("inf"))):
        d, ev, tr = dev.up(np.array([0.75])), dev.up(np.array([e] + [0.0] * 9)), dev.up(rec)
        out = dev.up(np.full(1 + nr.NSTATE + 2, SENTINEL))
        assert lib.ani_md_npt_check(d.data_ptr(), ev.data_ptr(), tr.data_ptr(), out.data_ptr(), None) == 0
        o, d, r = dev.down(out, d, tr)
        assert o[0] == want and d[0] == 0.0 and (o[1 + nr.NSTATE:] == SENTINEL).all()
        _same(o[1:1 + nr.NSTATE], rec, "the record behind the word"), _same(r, rec, "the record is read only")


# ---- the per-atom kernels ------------------------------------------------------------------------------------------------------
def _inputs(n, nghost, seed):
    rng = np.random.default_rng(7000 + 31 * seed + 1000 * nghost + n)
    mass = nh.MASSES[rng.integers(0, 7, n)]
    p = dict(x=rng.uniform(0.0, 20.0, (n, 3)), v=rng.normal(0.0, 0.01, (n, 3)), f=rng.normal(0.0, 15.0, (n, 3)), mass=mass,
             s=(0.5 * DT * nh.FTM2V) / mass, shift=rng.choice([-20.0, 0.0, 20.0], (nghost, 3)) * rng.uniform(0.9, 1.1, (1, 3)))
    p["xb"] = p["x"] + rng.normal(0.0, 0.05, (n, 3))
    ps = nr.init_record(np.zeros(3), np.full(3, 20.0), n)
    ps[nr.PS_FV], ps[nr.PS_MU] = 0.998046875 + 1e-9, 1.00146484375 - 1e-9
    ps[nr.PS_RATIO:nr.PS_RATIO + 3] = [1.0029296875, 0.9970703125 + 1e-10, 1.0 + 2.0 ** -30]
    ps[nr.PS_C:nr.PS_C + 3] = [10.0, 9.75, 10.5]
    ns = np.zeros(nh.NSTATE)
    ns[2] = 0.99873046875 + 1e-9
    p["ps"], p["ns"] = ps, ns
    return p


def _call_initial(dev, p, n, nghost, d2max=0.0, guard=3):
    """the kernel on n atoms and nghost shift rows, `guard` sentinel rows behind each"""
    g = np.full((guard, 3), SENTINEL)
    tx, tv, tf, ts, txb = (dev.up(np.concatenate([p[k], g]) if k in ("x", "v") else p[k]) for k in ("x", "v", "f", "s", "xb"))
    tsh = dev.up(np.concatenate([p["shift"], g]))
    d, tn, tp = dev.up(np.array([d2max])), dev.up(p["ns"]), dev.up(p["ps"])
    assert dev.lib.ani_md_npt_initial_integrate(tx.data_ptr(), tv.data_ptr(), tf.data_ptr(), ts.data_ptr(), DT, n, txb.data_ptr(),
                                                d.data_ptr(), tn.data_ptr(), tp.data_ptr(), tsh.data_ptr(), nghost, None) == 0
    return dev.down(tx, tv, tf, tsh, d, tn, tp)


@pytest.mark.parametrize("nghost", GHOSTS)
@pytest.mark.parametrize("n", SIZES)
def test_initial_integrate_and_the_shift_rows(n, nghost, dev):
    p = _inputs(n, nghost, 1)
    ps, ns = p["ps"], p["ns"]
    s, fv, mu, c = ns[2], ps[nr.PS_FV], ps[nr.PS_MU], ps[nr.PS_C:nr.PS_C + 3]
    runs = [_call_initial(dev, p, n, nghost) for _ in range(2)]
    for a, b, what in zip(runs[0], runs[1], ("x", "v", "f", "shift", "d2max", "NH record", "barostat record")):
        _same(a, b, f"two launches: {what}")
    x, v, f, sh, d, gn, gp = runs[0]
    xr, vr, dr = nr.npt_initial_integrate(p["x"], p["v"], p["f"], p["s"], DT, p["xb"], 0.0, s, fv, mu, c)
    mv = np.abs(s * fv * p["v"]) + p["s"][:, None] * np.abs(p["f"])
    mx = mu * mu * (2.0 * np.abs(c)[None, :] + np.abs(p["x"]) + np.abs(p["x"] - c[None, :]) + DT * mv)
    _within(v[:n], vr, 4, mv, "npt_initial_integrate v")
    _within(x[:n], xr, 12, mx, "npt_initial_integrate x")
    assert (x[n:] == SENTINEL).all() and (v[n:] == SENTINEL).all()
    _same(f, p["f"], "f is read only"), _same(gn, ns, "NH record is read only"), _same(gp, ps, "barostat record is read only")
    _same(sh[:nghost], nr.scale_shifts(p["shift"], ps[nr.PS_RATIO:nr.PS_RATIO + 3]), "shift rows")
    assert (sh[nghost:] == SENTINEL).all()
    bar = _d2_bar(xr, p["xb"], 12, mx)
    print(f"  n {n} nghost {nghost}: d2max {d[0]!r} against {dr!r}: off by {abs(d[0] - dr):.3e}, bar {bar:.3e}")
    assert abs(d[0] - dr) <= bar
    assert _call_initial(dev, p, n, nghost, d2max=1.0e6)[4][0] == 1.0e6          # a larger running maximum stays
    # s = fv = mu = 1: the positions and velocities of ani_md_initial_integrate to the rounding of c + (x - c)
    q = dict(p, ns=np.where(np.arange(nh.NSTATE) == 2, 1.0, 0.0), ps=nr.init_record(np.zeros(3), np.full(3, 20.0), n))
    x1, v1 = _call_initial(dev, q, n, nghost)[:2]
    x0, v0, _ = nr.mr.initial_integrate(p["x"], p["v"], p["f"], p["s"], DT, p["xb"], 0.0)
    _within(v1[:n], v0, 2, np.abs(p["v"]) + p["s"][:, None] * np.abs(p["f"]), "v with s = fv = mu = 1")
    assert np.abs(x1[:n] - x0).max() <= 12 * 2.0 ** -53 * 40.0


@pytest.mark.parametrize("n", SIZES)
def test_final_integrate_and_its_partials(n, dev):
    lib, torch = dev.lib, dev.torch
    p = _inputs(n, 0, 2)
    fv = p["ps"][nr.PS_FV]
    nblk = (n + 255) // 256
    vin = np.concatenate([p["v"], np.full((2, 3), SENTINEL)])
    outs = []
    for _ in range(2):
        tv, tf, ts, tm, tp = dev.up(vin), dev.up(p["f"]), dev.up(p["s"]), dev.up(p["mass"]), dev.up(p["ps"])
        w = torch.full((nblk + 3,), SENTINEL, dtype=torch.float64, device=dev.dev)
        assert lib.ani_md_npt_final_integrate(tv.data_ptr(), tf.data_ptr(), ts.data_ptr(), tm.data_ptr(), n, tp.data_ptr(), w.data_ptr(),
                                              None) == 0
        w2 = torch.full((nblk + 3,), SENTINEL, dtype=torch.float64, device=dev.dev)
        assert lib.ani_md_nh_kinetic(tv.data_ptr(), tm.data_ptr(), n, w2.data_ptr(), None) == 0
        outs.append(dev.down(tv, tf, w, w2, tp))
    for a, b, what in zip(outs[0], outs[1], ("v", "f", "partials", "nh_kinetic", "record")):
        _same(a, b, f"two launches: {what}")
    v, f, part, part2, gp = outs[0]
    vr, k2 = nr.npt_final_integrate(p["v"], p["f"], p["s"], p["mass"], fv)
    _within(v[:n], vr, 3, fv * (np.abs(p["v"]) + p["s"][:, None] * np.abs(p["f"])), "npt_final_integrate v")
    _same(v[n:], vin[n:], "rows behind nlocal"), _same(f, p["f"], "f is read only"), _same(gp, p["ps"], "record is read only")
    assert (part[nblk:] == SENTINEL).all()
    _same(part, part2, "partials of ani_md_npt_final_integrate against ani_md_nh_kinetic on its output")
    got, ref = math.fsum(part[:nblk].tolist()), nh.k2_sum(v[:n], p["mass"])
    assert abs(got - ref) <= (n + 16) * 2.0 ** -52 * ref
    # fv = 1: ani_md_nh_final_integrate bit for bit
    one = p["ps"].copy()
    one[nr.PS_FV] = 1.0
    tv, tv2, tf, ts, tm, tp = dev.up(p["v"]), dev.up(p["v"]), dev.up(p["f"]), dev.up(p["s"]), dev.up(p["mass"]), dev.up(one)
    w = torch.empty(nblk, dtype=torch.float64, device=dev.dev)
    assert lib.ani_md_npt_final_integrate(tv.data_ptr(), tf.data_ptr(), ts.data_ptr(), tm.data_ptr(), n, tp.data_ptr(), w.data_ptr(), None) == 0
    assert lib.ani_md_nh_final_integrate(tv2.data_ptr(), tf.data_ptr(), ts.data_ptr(), tm.data_ptr(), n, w.data_ptr(), None) == 0
    a, b = dev.down(tv, tv2)
    _same(a, b, "v with fv = 1 against ani_md_nh_final_integrate")


def test_no_owned_atoms_touch_nothing(dev):
    p = _inputs(4, 2, 3)
    x, v, f, sh, d, _, _ = _call_initial(dev, p, 0, 2, d2max=3.5, guard=0)
    _same(x, p["x"], "x"), _same(v, p["v"], "v"), _same(sh, p["shift"], "shift")
    assert d[0] == 3.5
    tv, tf, ts, tm, tp, w = (dev.up(a) for a in (p["v"], p["f"], p["s"], p["mass"], p["ps"], np.array([SENTINEL])))
    assert dev.lib.ani_md_npt_final_integrate(tv.data_ptr(), tf.data_ptr(), ts.data_ptr(), tm.data_ptr(), 0, tp.data_ptr(), w.data_ptr(),
                                              None) == 0
    v, w = dev.down(tv, w)
    _same(v, p["v"], "v"), _same(w, np.array([SENTINEL]), "partials")
