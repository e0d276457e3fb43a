"""CPU: the numpy reference of the isotropic barostat (tests/npt_reference.py, written from include/ani_md.h) on its own: the conserved
quantity it states is conserved to second order by the half-steps it states, it reduces to the thermostatted reference when the
barostat is infinitely heavy, its sign is right, its float64 form stays inside a tenth of the device bars against np.longdouble, and
the re-neighbouring limit of a moving box (lammps_ani_amd.md.npt_rebuild_limit) on corner moves made by hand.
"""
import numpy as np

import nh_reference as nh
import npt_reference as nr


def _run(dt, steps, every, **kw):
    x, v, m, lo, length, evaluate = nr.smooth_pair_system()
    args = dict(t_start=300.0, t_period=50.0, p_start=1.0, p_period=200.0)
    args.update(kw)
    out = nr.npt_trajectory(x, v, m, evaluate, steps, dt, lo, length, **args)
    return out[::every]


def test_conserved_quantity_is_second_order_and_the_recollected_form_is_not():
    """32 atoms, smooth pair potential, 2 ps at dt = 2 fs and 1 fs, read at the same instants.  The header's econserve (the barostat
    terms three times, p_target (V - V0) once) wanders at second order and far less than pe + ke; the other form (barostat terms once,
    p_target (V - V0) / 3) does not stay put under these half-steps."""
    w = {}
    for dt, every in ((2.0, 1), (1.0, 2)):
        rows = _run(dt, int(2000 / dt), every)
        c = np.array([r["econserve"] for r in rows])
        e = np.array([r["pe"] + r["ke"] for r in rows])
        other = np.array([r["pe"] + r["ke"] + float(r["chain"][4]) + (0.5 * r["baro"][nr.PS_W] * r["baro"][nr.PS_WD] ** 2 +
                          r["baro"][nr.PS_ECHAIN]) + r["p_target"] * (r["vol"] - r["baro"][nr.PS_V0]) / (3.0 * nh.NKTV2P) for r in rows])
        vols = np.array([r["vol"] for r in rows])
        w[dt] = (nh.wander(c), nh.wander(e), nh.wander(other))
        print(f"dt {dt}: wander econserve {w[dt][0]:.4f}, pe + ke {w[dt][1]:.2f}, other form {w[dt][2]:.2f}; V {vols.min():.1f} .. {vols.max():.1f}")
        assert nh.wander(vols) > 0.05 * vols[0]                    # the box breathed
        assert all(r["baro"][nr.PS_NONFINITE] == 0 and r["baro"][nr.PS_COUNT] == 2 * k * every for k, r in enumerate(rows))
    print(f"ratio {w[1.0][0] / w[2.0][0]:.3f}; econserve / (pe + ke) {w[2.0][0] / w[2.0][1]:.2e}")
    assert w[1.0][0] <= 0.3 * w[2.0][0]
    for dt in (2.0, 1.0):
        assert w[dt][0] <= 0.01 * w[dt][1]
        assert w[dt][2] > 10.0 * w[dt][0]                          # the form that is not conserved


def test_an_infinitely_heavy_barostat_is_the_thermostatted_trajectory():
    x, v, m, lo, length, evaluate = nr.smooth_pair_system()
    a = nr.npt_trajectory(x, v, m, evaluate, 40, 1.0, lo, length, 300.0, 450.0, 50.0, p_start=1.0, p_period=1e30)
    b = nh.nvt_trajectory(x, v, m, lambda xx: evaluate(xx, lo, length)[:2], 40, 1.0, 300.0, 450.0, 50.0)
    for k, (ra, rb) in enumerate(zip(a, b)):
        for key in ("x", "v", "f"):
            scale = np.abs(rb[key]).max()
            assert np.abs(ra[key] - rb[key]).max() <= 1e-12 * scale, key
        if k:                                                       # step 0: the thermostatted reference records its start sum
            assert np.allclose(ra["chain"], rb["chain"], rtol=1e-12, atol=0.0)
        assert (ra["len"] == length).all() and ra["baro"][nr.PS_MU] == 1.0 and ra["baro"][nr.PS_FV] == 1.0


def test_sign_the_volume_falls_towards_a_higher_target():
    x, v, m, lo, length, evaluate = nr.smooth_pair_system()
    p0 = nr.npt_trajectory(x, v, m, evaluate, 0, 1.0, lo, length, 300.0)[0]["press"]
    for dp, falls in ((+3000.0, True), (-3000.0, False)):
        rows = nr.npt_trajectory(x, v, m, evaluate, 30, 1.0, lo, length, 300.0, t_period=50.0, p_start=p0 + dp, p_period=200.0)
        print(f"pressure now {p0:.0f} atm, target {p0 + dp:.0f}: V {rows[0]['vol']:.2f} -> {rows[-1]['vol']:.2f}")
        assert (rows[-1]["vol"] < rows[0]["vol"]) == falls
        assert abs(rows[-1]["vol"] - rows[0]["vol"]) > 1e-3 * rows[0]["vol"]
        # omega is ln(L / L0), the box scales about c, and the record's volume is the box's
        r = rows[-1]["baro"]
        assert np.allclose(np.exp(r[nr.PS_OMEGA]), r[nr.PS_LEN] / length[0], rtol=1e-12)
        assert np.allclose(r[nr.PS_LO:nr.PS_LO + 3] + 0.5 * r[nr.PS_LEN:nr.PS_LEN + 3], r[nr.PS_C:nr.PS_C + 3], rtol=0, atol=1e-12)
        assert r[nr.PS_VOL] == nr.volume(r)


def test_the_pressure_ramp_ends_on_p_stop():
    rows = _run(1.0, 4, 1, p_start=100.0, p_stop=500.0)
    assert [r["p_target"] for r in rows[1:]] == [200.0, 300.0, 400.0, 500.0]
    assert rows[-1]["baro"][nr.PS_PTARGET] == 500.0


def test_float64_reference_against_longdouble_on_the_drawn_cases():
    """the reference in float64 stays within a tenth of the floors of half_step_bars of the reference in np.longdouble"""
    worst = 0.0
    for phase in (0, 1):
        for c in nr.npt_cases():
            ns, ps, bn, bp = nr.half_step_bars(phase, c)
            nl, pl, _ = nr.case_half_step(phase, c, np.longdouble)
            assert ps[nr.PS_NONFINITE] == 1.0 and ps[nr.PS_COUNT] == 7.0 and ns[0] == 8.0
            for got, ref, bar in ((ns, nl, bn), (ps, pl, bp)):
                err = np.abs(got - ref).astype(np.float64)
                assert (err <= bar).all()
                nz = bar > 0
                worst = max(worst, float((err[nz] / bar[nz]).max()))
                assert (err[~nz] == 0.0).all()
    print(f"largest |float64 - longdouble| as a fraction of the bar: {worst:.3f}")
    assert worst <= 0.1 + 1e-12


def test_non_finite_half_step_of_the_reference():
    c = nr.npt_cases()[0]
    ns, ps, _ = nr.half_step(0, c["ns"], c["ps"], c["K2"], float("inf"), c["t_target"], c["p_target"], c["tdof"], c["dt"], c["t_period"],
                             c["drag"], c["p_period"], c["M"], c["nc"], c["Mp"], c["ncp"])
    assert ns[2] == 1.0 and ps[nr.PS_FV] == 1.0 and ps[nr.PS_MU] == 1.0 and (ps[nr.PS_RATIO:nr.PS_RATIO + 3] == 1.0).all()
    assert ps[nr.PS_NONFINITE] == 2.0 and ns[6] == 3.0 and ps[nr.PS_COUNT] == 6.0 and ns[0] == 7.0
    keep = [nr.PS_WD, nr.PS_OMEGA] + list(range(nr.PS_LO, nr.PS_RATIO)) + list(range(nr.PS_ETA, nr.PS_ECHAIN))
    assert (ps[keep] == c["ps"][keep]).all() and (ns[8:] == c["ns"][8:]).all()


def test_rebuild_limit_on_corner_moves_made_by_hand():
    from lammps_ani_amd.md import npt_rebuild_limit
    lo, length, skin = np.zeros(3), np.full(3, 10.0), 2.0
    assert npt_rebuild_limit(skin, lo, length, lo, length, 1) == 1.0                 # a box at rest: (skin / 2)^2
    assert npt_rebuild_limit(skin, lo, length, lo, length, 2) == 1.0
    # the upper corner moves by (0.3, 0, 0.4): 0.5; the lower by (0, 0.1, 0): 0.1
    lo2, len2 = np.array([0.0, 0.1, 0.0]), np.array([10.3, 9.9, 10.4])
    assert np.isclose(npt_rebuild_limit(skin, lo, length, lo2, len2, 1), (0.5 * (2.0 - 0.6)) ** 2, rtol=1e-14)
    assert np.isclose(npt_rebuild_limit(skin, lo, length, lo2, len2, 2), (0.5 * (2.0 - 1.2)) ** 2, rtol=1e-14)
    assert npt_rebuild_limit(skin, lo, length, lo2, len2, 4) == 0.0                  # the clamp: any displacement rebuilds
    assert npt_rebuild_limit(skin, lo, length, lo - 1.0, length + 2.0, 1) == 0.0
    # an isotropic dilation about the centre by 1 %: both corners move by 0.05 sqrt(3)
    mu = 1.01
    got = npt_rebuild_limit(skin, lo, length, 5.0 + mu * (lo - 5.0), mu * length, 1)
    assert np.isclose(got, (0.5 * (2.0 - 2 * 0.05 * np.sqrt(3.0))) ** 2, rtol=1e-12)
    for args in ((lo, length, lo2, len2, 1), (lo, length, lo2, len2, 2), (lo, length, lo2, len2, 4)):
        assert npt_rebuild_limit(skin, *args) == nr.rebuild_limit(skin, *args)
    # why it is safe, on numbers: two atoms a skin apart beyond the cutoff at the build, across a face; each moves by less than the
    # square root of the limit and the image shift changes with the box -- they are still outside the cutoff
    cut = 5.1
    xa, xb = np.array([0.2, 5.0, 5.0]), np.array([10.0 - (cut + skin) + 0.2, 5.0, 5.0])
    assert np.isclose(np.linalg.norm(xa + np.array([10.0, 0, 0]) - xb), cut + skin)
    lo3, len3 = np.array([0.2, 0.0, 0.0]), np.array([9.6, 10.0, 10.0])                # the box shrank by 0.4 in x
    d = np.sqrt(npt_rebuild_limit(skin, lo, length, lo3, len3, 1))
    worst = np.linalg.norm((xa - np.array([d, 0, 0])) + np.array([len3[0], 0, 0]) - (xb + np.array([d, 0, 0])))
    assert worst >= cut - 1e-12
