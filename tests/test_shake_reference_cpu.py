"""CPU: the numpy RATTLE of tests/shake_reference.py meets its own contract, the input recipe of the kernel tests has the edges it
promises, and the package's cluster builder (lammps_ani_amd.md.constraint_clusters) agrees with the reference's.
"""
import numpy as np
import pytest

import shake_reference as sr


@pytest.mark.parametrize("nc", [1, 65, 257])
def test_reference_meets_its_own_constraints(nc):
    case, x, v, it, vr = sr.kernel_case_reference(nc)
    cl, d, L, w = case["cl"], case["d"], case["L"], case["w"]
    assert sr.residuals(case["x0"], cl, d, L).max() < 1e-13              # the start lies on the constraints
    assert sr.residuals(case["xp"], cl, d, L).max() > 1e-3               # the unconstrained move does not
    res = sr.residuals(x, cl, d, L).max()
    print(f"nc {nc}: {it.max()} iterations at most, residual {res:.2e} recomputed from 20 A coordinates")
    assert res <= 1e-13 and it.max() <= 10
    # sum_i m_i dx_i = 0 and sum_i m_i dv_i = 0 per cluster
    m = case["m"]
    for c in range(nc):
        atoms = [j for j in cl[c] if j >= 0]
        px = (m[atoms, None] * (x[atoms] - case["xp"][atoms])).sum(0)
        pv = (m[atoms, None] * (vr[atoms] - case["v"][atoms])).sum(0)
        assert np.abs(px).max() <= 1e-13 * m[atoms].max() and np.abs(pv).max() <= 1e-13 * m[atoms].max()
    # v += (x - x') / dt, the rest untouched
    assert np.abs(v - (case["v"] + (x - case["xp"]) / sr.DT)).max() <= 1e-15
    assert np.array_equal(x[case["free"]], case["xp"][case["free"]]) and np.array_equal(vr[case["free"]], case["v"][case["free"]])
    # r . dv = 0 after the velocity stage
    vmax = np.abs(vr).max()
    assert sr.velocity_defect(x, v, cl, L) > 1e-4 * vmax
    assert sr.velocity_defect(x, vr, cl, L) <= 1e-14 * vmax


@pytest.mark.parametrize("nc", sr.KERNEL_COUNTS)
def test_the_kernel_recipe_has_its_edges(nc):
    case = sr.kernel_case(nc)
    cl, x0 = case["cl"], case["x0"]
    assert 0 in case["straddling"]                                        # placed by hand: present at every size
    assert (x0 >= 0.0).all() and (x0 < sr.BOX).all()
    Ks = (cl[:, 1:] >= 0).sum(1)
    assert set(Ks.tolist()) <= {1, 2, 3} and (nc < 63 or set(Ks.tolist()) == {1, 2, 3})
    assert nc < 63 or (np.diff(Ks) != 0).any()                            # K in random order: a wave holds several sizes
    used = cl[cl >= 0]
    assert len(set(used.tolist())) == used.size and len(case["free"]) >= 1
    assert not set(case["free"].tolist()) & set(used.tolist())
    for c in range(nc):                                                   # any two bonds of a centre at least 60 degrees apart
        p = [j for j in cl[c, 1:] if j >= 0]
        r = sr.minimg(x0[cl[c, 0]] - x0[p], case["L"])
        u = r / np.sqrt((r * r).sum(1))[:, None]
        assert len(p) == 1 or (u @ u.T)[np.triu_indices(len(p), 1)].max() <= 0.5 + 1e-12


def test_the_start_projection_form_moves_onto_the_lengths():
    case = sr.kernel_case(65)
    d = case["d"] * 1.02                                                  # lengths that the positions do not have
    x, v, it, res = sr.shake_positions(case["x0"], None, case["cl"], d, case["w"], sr.DT, case["L"])
    assert v is None and sr.residuals(x, case["cl"], d, case["L"]).max() <= 1e-13 and it.min() >= 1
    x2, _, it2, _ = sr.shake_positions(x, None, case["cl"], d, case["w"], sr.DT, case["L"], tol=1e-12)
    assert it2.max() == 0 and np.array_equal(x2, x)                       # a start that holds takes no iteration and moves nothing


def _star_forest(rng, natoms, nclusters):
    tags = rng.permutation(10 * natoms)[:natoms] + 1
    atoms = rng.permutation(natoms)
    bonds, at = [], 0
    for _ in range(nclusters):
        K = int(rng.integers(1, 4))
        if at + 1 + K > natoms:
            break
        c, p = atoms[at], atoms[at + 1: at + 1 + K]
        at += 1 + K
        for j in p:
            bonds.append((tags[c], tags[j]) if rng.random() < 0.5 else (tags[j], tags[c]))
    order = rng.permutation(len(bonds))
    return tags, np.array(bonds, dtype=np.int64)[order]


@pytest.mark.parametrize("seed", range(6))
def test_package_cluster_builder_agrees_with_the_reference(seed):
    from lammps_ani_amd import md
    rng = np.random.default_rng(seed)
    tags, bonds = _star_forest(rng, 400, 90)
    cl, slot = md.constraint_clusters(bonds, tags)
    cl_ref, slot_ref = sr.build_clusters(bonds, tags)
    assert cl.dtype == np.int32 and cl.shape == (cl_ref.shape[0], 4) and slot.shape == (cl.shape[0], 3)
    assert sr.canonical(cl) == sr.canonical(cl_ref)
    K = (cl[:, 1:] >= 0).sum(1)
    assert (np.diff(K) >= 0).all()                                        # by size ...
    for k in (1, 2, 3):
        assert (np.diff(cl[K == k, 0]) > 0).all()                         # ... then by centre index
    assert ((cl[:, 1:] >= 0) == (slot >= 0)).all() and (np.sort(slot[slot >= 0]) == np.arange(len(bonds))).all()
    for c in range(cl.shape[0]):                                          # every slot names the bond it came from
        for k in range(3):
            if slot[c, k] >= 0:
                assert {int(tags[cl[c, 0]]), int(tags[cl[c, 1 + k]])} == set(bonds[slot[c, k]].tolist())
    # used slots first, -1 behind them
    assert ((cl[:, 1:] >= 0) == (np.arange(3)[None, :] < K[:, None])).all()


@pytest.mark.parametrize("what, bonds, tag", [
    ("chain of four", [(1, 2), (2, 3), (3, 4)], r"\b(2|3)\b"),
    ("ring", [(1, 2), (2, 3), (3, 1)], r"\b(1|2|3)\b"),
    ("four partners", [(5, 1), (5, 2), (5, 3), (5, 4)], r"\b5\b"),
    ("duplicate", [(1, 2), (3, 4), (2, 1)], r"\b(1|2)\b.*\b(1|2)\b"),
    ("self-bond", [(1, 2), (3, 3)], r"\b3\b"),
    ("unknown tag", [(1, 2), (3, 77)], r"\b77\b"),
])
def test_builders_raise_on_malformed_input(what, bonds, tag):
    from lammps_ani_amd import md
    tags = np.array([4, 3, 2, 1, 5, 6])
    for build in (md.constraint_clusters, sr.build_clusters):
        with pytest.raises(ValueError, match=tag):
            build(np.array(bonds), tags)


def test_two_atom_component_and_empty_list():
    from lammps_ani_amd import md
    cl, slot = md.constraint_clusters(np.array([(7, 9)]), np.array([9, 8, 7]))
    assert sorted(cl[0, :2].tolist()) == [0, 2] and cl[0, 2:].tolist() == [-1, -1] and slot.tolist() == [[0, -1, -1]]
    cl, slot = md.constraint_clusters(np.zeros((0, 2), dtype=np.int64), np.arange(5))
    assert cl.shape == (0, 4) and slot.shape == (0, 3)
