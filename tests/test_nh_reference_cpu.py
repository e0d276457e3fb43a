"""CPU: the Nose-Hoover chain reference (tests/nh_reference.py) on its own -- the conserved quantity of an oracle-driven trajectory,
the chain's limiting cases, the target ramp, its rounding against an evaluation in np.longdouble -- and the two host functions of
the built library that need no device.
"""
import functools
import os

import numpy as np

import nh_reference as nh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _trajectory(model_path, dt, steps, t_target=nh.T_TARGET):
    s, m, v0 = nh.water30(ROOT)
    return nh.nvt_trajectory(s.x, v0, m, nh.oracle_evaluator(model_path, s), steps, dt, t_target, None, nh.T_PERIOD, nh.MTCHAIN)


def test_conserved_quantity_is_second_order_and_far_below_the_energy_exchanged(model_cache):
    """30-atom water box, 300 K start, target 600 K, t_period 20 fs, three links, 50 fs: the wander (max - min) of
    pe + ke + ecouple at dt 0.25 fs is at most half of that at 0.5 fs (second order: a quarter), and at most 0.01 of the wander of
    pe + ke, which the thermostat heats by about 96 kcal/mol.  Measured: 0.156 and 0.044 kcal/mol (ratio 0.28), 0.0016 of 97.6."""
    path = model_cache(*nh.WATER_MODEL)
    w = {}
    for dt, steps in ((0.5, 100), (0.25, 200)):
        tr = _trajectory(path, dt, steps)
        e = np.array([r["pe"] + r["ke"] for r in tr])
        w[dt] = (nh.wander(e + np.array([r["ecouple"] for r in tr])), nh.wander(e))
        assert tr[-1]["chain"][0] == 2 * steps
    print(f"wander of pe + ke + ecouple: {w[0.5][0]:.4f} (dt 0.5), {w[0.25][0]:.4f} (dt 0.25), ratio {w[0.25][0] / w[0.5][0]:.3f}; "
          f"of pe + ke: {w[0.5][1]:.2f}, {w[0.25][1]:.2f}")
    assert w[0.25][0] <= 0.5 * w[0.5][0]
    for dt in (0.5, 0.25):
        assert w[dt][0] <= 0.01 * w[dt][1]
    assert w[0.5][1] > 50.0                                     # the thermostat did heat the box


def test_one_link_is_the_chain_with_the_upper_links_cut():
    """mtchain = 1 against link 0 written out alone (all it reads of the links above is eta_dot[1], which is 0 for a chain of
    one: e = 1), bit for bit; and against a longer chain whose upper links are at rest when the half-step begins, which link 0
    cannot tell from a chain of one within a single sub-step."""
    rng = np.random.default_rng(11)
    for _ in range(50):
        c = nh.draw_chain_case(rng)
        one = nh.chain_half_step(c["K2"], c["t_target"], c["tdof"], c["dt"], c["t_period"], c["drag"], 1, c["nc"], c["eta"][:1],
                                 c["eta_dot"][:1], c["eta_dotdot"][:1])
        # by hand: link 0 alone, e = exp(0) = 1
        kt, ket, Q = nh.chain_masses(c["t_target"], c["tdof"], c["t_period"], 1)
        nf = 1.0 / c["nc"]
        dfac, h2, h4 = 1.0 - c["dt"] * c["drag"] / c["nc"], nf * c["dt"] / 2.0, nf * c["dt"] / 4.0
        K2, eta, ed, s = c["K2"], c["eta"][0], c["eta_dot"][0], 1.0
        edd = (K2 - ket) / Q[0]
        for _ in range(c["nc"]):
            ed = (ed + edd * h4) * dfac
            fac = np.exp(-h2 * ed)
            s, K2 = s * fac, K2 * (fac * fac)
            edd = (K2 - ket) / Q[0]
            eta = eta + h2 * ed
            ed = ed + edd * h4
        assert (one["s"], one["K2"], one["eta"][0], one["eta_dot"][0], one["eta_dotdot"][0]) == (s, K2, eta, ed, edd)
        assert one["ecouple"] == ket * eta + 0.5 * Q[0] * ed * ed
        if c["M"] >= 2:
            ed_in = c["eta_dot"].copy()
            ed_in[1:] = 0.0
            edd_in = c["eta_dotdot"].copy()
            edd_in[1:] = 0.0
            full = nh.chain_half_step(c["K2"], c["t_target"], c["tdof"], c["dt"], c["t_period"], c["drag"], c["M"], 1, c["eta"], ed_in,
                                      edd_in)
            cut = nh.chain_half_step(c["K2"], c["t_target"], c["tdof"], c["dt"], c["t_period"], c["drag"], 1, 1, c["eta"][:1],
                                     ed_in[:1], edd_in[:1])
            assert full["s"] == cut["s"] and full["K2"] == cut["K2"] and full["eta"][0] == cut["eta"][0]


def test_chain_at_rest_on_target_does_not_scale():
    for tdof, T, M in ((87.0, 300.0, 1), (87.0, 300.0, 3), (300003.0, 612.5, 8)):
        ket = float(nh.chain_masses(T, tdof, 50.0, M)[1])
        z = np.zeros(M)
        r = nh.chain_half_step(ket, T, tdof, 0.5, 50.0, 0.0, M, 2, z, z, z)
        assert r["s"] == 1.0 and r["K2"] == ket and r["eta"][0] == 0.0 and r["eta_dot"][0] == 0.0 and r["eta_dotdot"][0] == 0.0
        if M > 1:   # link 1 feels -kt / Q[1] = -1 / t_period^2 and starts to move; the particles do not notice in this half-step
            assert np.isclose(r["eta_dotdot"][1], -1.0 / 50.0 ** 2, rtol=1e-12) and r["eta_dot"][1] < 0.0


def test_ramp_reaches_t_stop_at_step_n():
    for n, a, b in ((1, 300.0, 600.0), (7, 300.0, 600.0), (100, 123.4, 77.7), (3, 0.1, 0.3)):
        t = [nh.ramp_target(k, n, a, b) for k in range(1, n + 1)]
        assert t[-1] == b
        assert np.allclose(t, a + np.arange(1, n + 1) / n * (b - a), rtol=1e-15)
        assert all((x - a) * (b - x) >= 0.0 for x in t)
    m = np.array([1.008, 15.999, 1.008, 12.011])
    v = np.random.default_rng(5).normal(0.0, 0.01, (4, 3))
    tr = nh.nvt_trajectory(np.zeros((4, 3)), v, m, lambda x: (np.zeros_like(x), 0.0), 8, 0.5, 300.0, 600.0, 20.0, 2)
    assert [r["t_target"] for r in tr[1:]] == [nh.ramp_target(k, 8, 300.0, 600.0) for k in range(1, 9)]
    assert tr[-1]["chain"][3] == 600.0 and tr[-1]["chain"][0] == 16


def test_run_and_step_forms_differ_only_by_the_rounding_of_k2():
    """K2 carried through the chain's own scaling (run) against K2 summed again from the scaled velocities (step)"""
    m = nh.MASSES[np.random.default_rng(1).integers(0, 4, 40)]
    v = np.random.default_rng(2).normal(0.0, 0.01, (40, 3))
    x = np.random.default_rng(3).uniform(0.0, 8.0, (40, 3))
    force = lambda xx: (30.0 * np.sin(2.0 * np.pi * xx / 8.0 + np.arange(40)[:, None]), 0.0)
    a = nh.nvt_trajectory(x, v, m, force, 20, 0.5, 600.0, None, 20.0, 3, fresh_k2_every_step=True)
    b = nh.nvt_trajectory(x, v, m, force, 20, 0.5, 600.0, None, 20.0, 3, fresh_k2_every_step=False)
    assert np.allclose(a[-1]["v"], b[-1]["v"], rtol=1e-12, atol=0.0) and np.allclose(a[-1]["chain"], b[-1]["chain"], rtol=1e-12, atol=1e-18)


def test_float64_reference_against_its_longdouble_evaluation():
    """The reference's own rounding on the drawn inputs of the device test, as a fraction of that test's bars: a tenth at most
    (the device bars are ten times the reference's rounding).  Measured on x86-64 (80-bit long double): eta 8e-16 of max(1, |eta|),
    eta_dot 1.1e-14, eta_dotdot 4.4e-14, s / K2 / ecouple 9e-16 of their scales.  The cases are exactly those of the device test
    (nh_reference.chain_cases).  ecouple is the entry closest to its tenth: its rounding is that of eta_dot[0], squared in
    Q[0] eta_dot[0]^2 / 2, and over 2000 draws of the same recipe its tail reaches 1.08e-15 (99.9th percentile 9.6e-16)."""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than double here"
    worst = dict(eta=0.0, eta_dot=0.0, eta_dotdot=0.0, s=0.0, K2=0.0, ecouple=0.0)
    for c in nh.chain_cases():
        args = (c["K2"], c["t_target"], c["tdof"], c["dt"], c["t_period"], c["drag"], c["M"], c["nc"], c["eta"], c["eta_dot"],
                c["eta_dotdot"])
        r, q = nh.chain_half_step(*args), nh.chain_half_step(*args, dtype=np.longdouble)
        bars = nh.chain_bars(c, r)
        for key in worst:
            err = np.abs(np.asarray(r[key], dtype=np.longdouble) - q[key]).astype(np.float64)
            worst[key] = max(worst[key], float(np.max(err / bars[key])))
    print("largest |float64 - longdouble| as a fraction of the device bar:", {k: f"{w:.3f}" for k, w in worst.items()})
    for key, w in worst.items():
        assert w <= 0.1, (key, w)


def test_work_sizes_answer_through_the_built_library():
    from lammps_ani_amd import ani_hip
    lib = ani_hip.lib()
    for n, blocks in ((0, 1), (1, 1), (255, 1), (256, 1), (257, 2), (513, 3), (65537, 257), (100002, 391)):
        assert lib.ani_md_nh_work_size(n) == blocks
        assert lib.ani_md_thermo_work_size(n) == 6 * blocks
    assert ani_hip.NH_NSTATE == nh.NSTATE and ani_hip.THERMO_N == nh.THERMO_N and ani_hip.NH_MAXCHAIN == nh.MAXCHAIN
