"""CPU: the numpy FIRE of tests/fire_reference.py and the inputs of the GPU tests that compare against it.  Runs none of the
device code: the calculators are a separable quadratic and the CPU oracle."""
import numpy as np
import pytest

import fire_reference as fr


def test_reference_converges_on_a_separable_quadratic_and_never_climbs_after_a_downhill_test():
    rng = np.random.default_rng(42)
    n = 257
    x0 = rng.uniform(0.0, 20.0, (n, 3))
    kk = rng.uniform(200.0, 800.0, (n, 1))
    fm = fr.FTM2V / fr.MASSES[rng.integers(0, 7, n)]
    fire = fr.Fire(fr.fire_defaults(0.5, 0.0, 1e-5, 5000), fm)
    x, hist = fire.run(lambda x: (-kk * (x - x0), float(0.5 * (kk * (x - x0) ** 2).sum())), x0 + rng.normal(0.0, 0.08, (n, 3)))
    assert fire.stop == 2 and hist[-1]["what"] == "stop" and fire.ff < 1e-10
    assert 20 < fire.iterations < 3000
    assert fire.uphill >= 2 and any(b["dt"] > a["dt"] for a, b in zip(hist, hist[1:]))
    assert np.abs(x - x0).max() < 1e-6
    # A call that tests P > 0 moves along one straight line (an uphill call steps half a move back first).  P > 0 in the call after
    # it says that at the end of that line the energy still fell along it; the well is convex, so it fell all the way: over a
    # move that follows a P > 0 test and is followed by one, the energy does not rise.  (Where the next test finds P <= 0 the
    # move has overshot: that is what the test is for.)
    climbs = [j for j in range(1, len(hist)) if hist[j]["what"] == "downhill" and hist[j - 1]["what"] == "downhill"
              and hist[j]["E"] > hist[j - 1]["E"]]
    assert not climbs, climbs[:5]
    assert sum(h["what"] == "downhill" for h in hist) > 0.8 * len(hist)
    assert hist[-1]["E"] < 1e-9 * hist[0]["E"]


def test_reference_stops_by_etol_and_by_maxiter_and_freezes():
    rng = np.random.default_rng(1)
    x0 = rng.uniform(0.0, 5.0, (20, 3))
    fm = np.full(20, fr.FTM2V / 12.011)
    ev = lambda x: (-300.0 * (x - x0), float(150.0 * ((x - x0) ** 2).sum()) - 50.0)
    for params, code in ((fr.fire_defaults(0.5, 1e-10, 0.0, 5000), 1), (fr.fire_defaults(0.5, 0.0, 0.0, 17), 3)):
        fire = fr.Fire(params, fm)
        x, hist = fire.run(ev, x0 + 0.05)
        assert fire.stop == code and (code != 3 or fire.iterations == 17)
        before = (x.copy(), dict(fire.state()))
        v = np.ones_like(x)
        assert fire.iterate(x, v, np.ones_like(x), 3.0) == "frozen"
        assert np.array_equal(x, before[0]) and fire.state() == before[1] and (v == 1.0).all()
    fire = fr.Fire(fr.fire_defaults(0.5, 0.0, 0.0, 10), fm)
    assert fire.iterate(x0.copy(), np.zeros_like(x0), np.zeros_like(x0), float("nan")) == "stop" and fire.stop == 4


@pytest.mark.parametrize("name", sorted(fr.ORACLE_CASES))
def test_oracle_driven_cases_exercise_the_branches_with_a_margin(name, model_cache):
    sysm, p, hist = fr.oracle_case_run(name, model_cache("ani2x", 8, 2024))
    K = fr.ORACLE_CASES[name]["K"]
    assert len(hist) == K + 1 and hist[-1]["what"] == "stop" and hist[-1]["stop"] == 3 and hist[-1]["iterations"] == K
    moves = hist[:K]
    assert moves[0]["what"] == "uphill" and moves[0]["P"] == 0.0                    # the start from rest
    assert any(h["what"] == "uphill" for h in moves[1:])                             # an uphill event after iteration 1
    assert any(b["dt"] > a["dt"] for a, b in zip(moves, moves[1:]))                  # dt grew
    worst = min(abs(h["P"]) / np.sqrt(h["vv"] * h["ff"]) for h in hist if h["vv"] > 0)
    print(f"{name}: uphill {hist[-1]['uphill']}, limited {hist[-1]['limited']}, smallest |P| / sqrt(vv ff) {worst:.3f}, "
          f"E {hist[0]['E']:.4f} -> {hist[-1]['E']:.4f}, |f| {np.sqrt(hist[0]['ff']):.3f} -> {np.sqrt(hist[-1]['ff']):.3f}")
    assert worst >= 0.05                                    # no branch hangs on rounding-level force differences
    assert hist[-1]["E"] < hist[0]["E"] and hist[-1]["ff"] < hist[0]["ff"]
    if name == "water30":
        assert hist[-1]["limited"] >= 1                     # the dmax limit is taken in one of the cases


def test_the_larger_case_is_two_blocks_with_two_atoms_in_the_second():
    assert fr.case_system("water258").natoms == 258 and fr.case_system("water30").natoms == 30
