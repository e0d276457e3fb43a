"""CPU: the numpy reference of the umbrella restraints (tests/restraint_reference.py) against what defines it: the sign pin of the
torsion, central differences, the sum rules of forces and virial, invariance under box vectors, the fold of a torsion's difference,
the non-finite rule, and energy conservation of a restrained NVE run on npt_reference.smooth_pair_system."""
import numpy as np
import pytest

import nh_reference as nh
import npt_reference as nr
import restraint_reference as rr

L3 = np.array([11.0, 12.5, 10.0])
KINDS = (rr.DISTANCE, rr.ANGLE, rr.TORSION)


def _case(kind, seed):
    """a well-conditioned restraint of `kind` that sits across the faces of the box L3: (p [4, 3], kappa, centre)"""
    c = rr.chain_case(4, seed, L=10.0)
    chain = [int(c["atoms"][i][0]) for i in range(4)]        # restraint i starts at chain atom i
    p = c["x"][chain] + np.array([10.3, -0.4, 9.1])
    p = np.mod(p, L3)
    return p, 24.0, 0.4 + 0.1 * seed


@pytest.mark.parametrize("t", [-3.0, -1.2, -0.1, 0.0, 0.7, 1.5707963, 2.9, 3.14])
def test_the_sign_pin_of_the_torsion(t):
    p = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [np.cos(t), np.sin(t), 1.0]])
    cv, _, _, _ = rr.collective_variable(rr.TORSION, p, np.full(3, 50.0))
    assert abs(cv - t) <= 1e-15 * 8


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_gradients_against_central_differences(kind, seed):
    p, _, _ = _case(kind, seed)
    na, h = rr.NATOMS_OF[kind], 1e-6
    _, g, _, _ = rr.collective_variable(kind, p, L3)
    num = np.zeros((4, 3))
    for m in range(na):
        for k in range(3):
            pp, pm = p.copy(), p.copy()
            pp[m, k] += h
            pm[m, k] -= h
            d = rr.collective_variable(kind, pp, L3)[0] - rr.collective_variable(kind, pm, L3)[0]
            d -= rr.TWOPI * np.rint(d / rr.TWOPI) if kind == rr.TORSION else 0.0
            num[m, k] = d / (2.0 * h)
    scale = np.abs(g).max()
    assert scale > 0.1
    assert np.abs(g - num).max() <= 1e-7 * scale, np.abs(g - num).max() / scale
    assert (g[na:] == 0.0).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sum_rules_of_forces_and_virial(kind, seed):
    p, kap, _ = _case(kind, seed)
    na = rr.NATOMS_OF[kind]
    atoms = np.array([[0, 1, 2, 3]])
    atoms[0, na:] = -1
    cv0 = rr.collective_variable(kind, p, L3)[0]
    ev = rr.evaluate(p, atoms, [kind], [kap], [cv0 - 0.35], L3)
    f, w = ev["fslot"][0], ev["w"][0].reshape(3, 3)
    fs = np.abs(f).max()
    assert fs > 1.0 and ev["nonfinite"] == 0
    assert np.abs(f.sum(0)).max() <= 1e-13 * fs
    ws = np.abs(w).max() + ev["w_mag"][0].max()
    assert np.abs(w - w.T).max() <= 1e-13 * ws
    want = -kap * float(ev["delta"][0]) * float(cv0) if kind == rr.DISTANCE else 0.0
    assert abs(np.trace(w) - want) <= 1e-13 * ws
    assert np.isclose(float(ev["delta"][0]), 0.35, rtol=0, atol=1e-14) and np.isclose(float(ev["e"][0]), 0.5 * kap * 0.35 ** 2, rtol=1e-12)


@pytest.mark.parametrize("kind", KINDS)
def test_moving_an_atom_by_a_box_vector_changes_nothing(kind):
    p, kap, _ = _case(kind, 2)
    na = rr.NATOMS_OF[kind]
    atoms = np.array([[0, 1, 2, 3]])
    atoms[0, na:] = -1
    cen = rr.collective_variable(kind, p, L3)[0] + 0.2
    a = rr.evaluate(p, atoms, [kind], [kap], [cen], L3)
    for m in range(na):
        for shift in ((1, 0, 0), (0, -1, 0), (0, 0, 2), (-1, 1, -1)):
            q = p.copy()
            q[m] += np.array(shift) * L3
            b = rr.evaluate(q, atoms, [kind], [kap], [cen], L3)
            assert abs(b["cv"][0] - a["cv"][0]) <= 1e-13 and np.abs(b["fslot"] - a["fslot"]).max() <= 1e-12 * np.abs(a["fslot"]).max()
            assert np.abs(b["w"] - a["w"]).max() <= 1e-12 * np.abs(a["w"]).max()
    # a non-periodic dimension is not folded
    q = p.copy()
    q[0, 2] += L3[2]
    assert abs(rr.evaluate(q, atoms, [kind], [kap], [cen], L3, pmask=3)["cv"][0] - a["cv"][0]) > 1e-3


def test_the_fold_of_a_torsion_difference():
    assert np.isclose(rr.fold_delta(-rr.PI + 0.1, rr.PI - 0.1, rr.TORSION), 0.2, rtol=0, atol=1e-15)
    assert np.isclose(rr.fold_delta(rr.PI - 0.1, -rr.PI + 0.1, rr.TORSION), -0.2, rtol=0, atol=1e-15)
    assert rr.fold_delta(0.0, rr.PI, rr.TORSION) == rr.PI                 # (-pi, pi]: -pi folds to +pi
    assert np.isclose(rr.fold_delta(-rr.PI + 0.1, rr.PI - 0.1, rr.ANGLE), -rr.TWOPI + 0.2)   # only torsions fold
    t = -rr.PI + 0.1
    p = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [np.cos(t), np.sin(t), 1.0]])
    ev = rr.evaluate(p, [[0, 1, 2, 3]], [rr.TORSION], [10.0], [rr.PI - 0.1], np.full(3, 50.0))
    assert np.isclose(float(ev["delta"][0]), 0.2, atol=1e-14) and np.isclose(float(ev["e"][0]), 0.2, rtol=1e-12)


def test_a_collinear_torsion_is_nan_and_counted():
    x = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [3.0, 0, 0], [1.0, 1.0, 0.0], [2.0, 1.5, 0.5]])
    atoms = [[0, 1, 2, 3], [0, 1, -1, -1], [0, 4, 5, 3]]
    ev = rr.evaluate(x, atoms, [rr.TORSION, rr.DISTANCE, rr.TORSION], [10.0, 10.0, 10.0], [0.5, 0.5, 0.5], np.full(3, 50.0))
    assert ev["nonfinite"] == 1 and np.isnan(ev["e"][0]) and np.isnan(ev["E"])
    assert (ev["fslot"][0] == 0.0).all() and (ev["w"][0] == 0.0).all() and np.isfinite(ev["e"][1:]).all() and np.isfinite(ev["facc"]).all()
    # coincident atoms and a straight angle as well
    ev = rr.evaluate(x[[0, 0, 1, 2]], [[0, 1, -1, -1], [0, 2, 3, -1]], [rr.DISTANCE, rr.ANGLE], [1.0, 1.0], [1.0, 1.0], np.full(3, 50.0))
    assert ev["nonfinite"] == 2


def test_nve_conservation_with_restraints():
    """pe + bias + ke on the analytic pair system with two torsions that share three atoms and a distance: 200 fs at 2 fs and 1 fs;
    the wander falls with dt^2 (measured: 0.0094 and 0.00235 kcal/mol, ratio 0.25) while the bias moves by several kcal/mol"""
    x0, v0, m, lo, length, model = nr.smooth_pair_system()
    tors = [(0, 1, 5, 4), (1, 5, 4, 8)]
    start = rr.evaluate(x0, *rr.tables([("torsion", t, 0.0, 0.0) for t in tors] + [("distance", (2, 3), 0.0, 0.0)]), length)["cv"]
    restraints = [("torsion", tors[0], 24.0, float(start[0]) + 0.5), ("torsion", tors[1], 24.0, float(start[1]) + 0.5),
                  ("distance", (2, 3), 50.0, float(start[2]) - 0.3)]

    def total(x):
        f, pe, _ = model(x, lo, length)
        fb, eb, _, _ = rr.bias(x, restraints, length)
        total.bias.append(eb)
        return f + fb, pe + eb

    w = {}
    for dt in (2.0, 1.0):
        total.bias = []
        traj = rr.nve_trajectory(x0, v0, m, total, int(round(200.0 / dt)), dt)
        w[dt] = nh.wander(np.array([r["pe"] + r["ke"] for r in traj]))
        b = np.array(total.bias)
        print(f"dt {dt}: wander {w[dt]:.5f} kcal/mol, bias {b.min():.2f} .. {b.max():.2f}")
        assert b.max() - b.min() > 1.0
    print(f"ratio {w[1.0] / w[2.0]:.3f}")
    assert w[1.0] <= 0.3 * w[2.0]
