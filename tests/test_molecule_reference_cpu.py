"""CPU: the molecule finder's reference (tests/molecule_reference.py) against brute force over all pairs with the minimum image,
formula_string on hand-written cases, and what ani_set_bond_table can refuse without a device."""
import ctypes as C

import numpy as np
import pytest

import molecule_reference as mr
from lammps_ani_amd import harness as hx

TABLE = mr.load_table()


def _brute(sysm, table):
    """bond matrix of the whole periodic system: minimum image, all pairs (the box is wider than twice the longest bond)"""
    L = sysm.boxhi - sysm.boxlo
    assert L.min() > 2 * table.max()
    d = sysm.x[None, :, :] - sysm.x[:, None, :]
    d -= L * np.round(d / L)
    r2 = (d * d).sum(-1)
    sp = sysm.types.astype(np.int64) - 1
    cut = table[sp[:, None], sp[None, :]]
    bond = (r2 <= cut * cut) & (cut > 0)
    np.fill_diagonal(bond, False)
    return bond


def _components(bond, members):
    """label (smallest member) of every member under the bonds among the members"""
    label = {}
    for a in members:
        if a in label:
            continue
        comp, todo = {a}, [a]
        while todo:
            u = todo.pop()
            for v in np.nonzero(bond[u])[0].tolist():
                if v in members and v not in comp:
                    comp.add(v)
                    todo.append(v)
        for u in comp:
            label[u] = min(comp)
    return label


def test_fixture_table():
    sym = list(mr.SYMBOLS_ANI2X)
    assert TABLE.shape == (7, 7) and np.array_equal(TABLE, TABLE.T)
    assert TABLE[sym.index("H"), sym.index("O")] == pytest.approx(1.16) and TABLE[sym.index("O"), sym.index("O")] == pytest.approx(1.68)
    assert TABLE[sym.index("C"), sym.index("N")] == pytest.approx(1.63)
    assert (TABLE[4:] == 0).all()   # S, F, Cl: not in the analysis table, never bonded
    assert TABLE.max() < 3.5


@pytest.mark.parametrize("n,L,seed", [(60, 8.0, 1), (48, 7.5, 2), (60, 7.2, 5)])
def test_reference_equals_brute_force_one_rank(n, L, seed):
    sysm = hx.random_box(n, 4, L, seed=seed)
    inp = hx.decompose(sysm)
    assert inp.nlocal == n and np.array_equal(inp.tag[:n], np.arange(n))
    labels, formulas, summary, image = mr.find_molecules(inp, TABLE, mr.owners_of(inp))
    bond = _brute(sysm, TABLE)
    want = _components(bond, set(range(n)))
    assert [want[a] for a in range(n)] == labels.tolist()
    sp = sysm.types.astype(np.int64) - 1
    comps = {}
    for r in set(want.values()):
        c = tuple(np.bincount(sp[[a for a in range(n) if want[a] == r]], minlength=7).tolist())
        comps[c] = comps.get(c, 0) + 1
    assert comps == formulas
    sizes = np.bincount(labels)
    assert summary.tolist() == [len(set(want.values())), len(comps), 0, int(bond.sum()), int(sizes.max()), 0]
    assert summary[0] < n and image > 0   # the boxes are dense enough to bond, small enough to bond through a face
    assert np.array_equal(mr.formula_rows(formulas)[:, -1].sum(), summary[0])


@pytest.mark.parametrize("rank", [0, 1])
def test_reference_equals_brute_force_two_ranks(rank):
    sysm = hx.random_box(60, 4, 8.0, seed=1)
    inp = hx.decompose(sysm, grid=(2, 1, 1), rank=rank)
    nl = inp.nlocal
    labels, formulas, summary, _ = mr.find_molecules(inp, TABLE, mr.owners_of(inp, rank))
    bond = _brute(sysm, TABLE)
    tag = inp.tag[:nl].tolist()
    mine = set(tag)
    want = _components(bond, mine)
    # the label is the smallest LOCAL index of the component (local order need not follow the tags)
    assert [min(k for k, u in enumerate(tag) if want[u] == want[t]) for t in tag] == labels.tolist()
    open_roots = {want[t] for t in tag if any(v not in mine for v in np.nonzero(bond[t])[0].tolist())}
    assert open_roots, "the cut must go through a molecule"
    assert summary[2] == len(open_roots)
    assert summary[5] == sum(1 for t in tag if want[t] in open_roots)
    sp = sysm.types.astype(np.int64) - 1
    comps = {}
    for r in set(want.values()) - open_roots:
        c = tuple(np.bincount(sp[[t for t in tag if want[t] == r]], minlength=7).tolist())
        comps[c] = comps.get(c, 0) + 1
    assert comps == formulas
    assert summary[0] == len(set(want.values())) and summary[3] == int(bond[tag].sum())
    # every ghost foreign: at least as many open molecules
    assert mr.find_molecules(inp, TABLE, None)[2][2] >= summary[2]


def test_formula_string():
    from lammps_ani_amd.ani_hip import formula_dict, formula_string
    sym = ["H", "C", "N", "O", "S", "F", "Cl"]
    assert formula_string([4, 1, 0, 0, 0, 0, 0], sym) == "CH4"
    assert formula_string([0, 0, 0, 2, 0, 0, 0], sym) == "O2"
    assert formula_string([2, 0, 0, 1, 0, 0, 0], sym) == "H2O"
    assert formula_string([0, 1, 0, 1, 0, 0, 0], sym) == "CO"
    assert formula_string([0, 1, 0, 2, 0, 0, 0], sym) == "CO2"
    assert formula_string([1, 0, 0, 0, 0, 0, 0], sym) == "H"
    assert formula_string([5, 2, 1, 2, 0, 0, 0], sym) == "C2H5NO2"          # glycine: C, H, then alphabetical
    assert formula_string([1, 1, 0, 0, 1, 1, 3], sym) == "CHCl3FS"          # Cl sorts before F before S
    assert formula_string([1, 0, 1, 3, 0, 0, 0], sym) == "HNO3"             # no carbon: H still first
    assert formula_string([0, 600, 0, 0, 0, 0, 0], sym) == "C600"
    assert formula_string([0] * 7, sym) == ""
    assert formula_string([2, 1], ["O", "H"]) == "HO2"                      # by symbol, not by species order
    assert formula_dict(np.array([[4, 1, 0, 0, 128], [0, 0, 0, 2, 256]]), ["H", "C", "N", "O"]) == {"CH4": 128, "O2": 256}


def test_entry_points_refuse_a_null_handle():
    """the only argument check that needs no device (there is no handle without one)"""
    from lammps_ani_amd import ani_hip
    lib = ani_hip.lib()
    t = np.zeros((7, 7))
    assert lib.ani_set_bond_table(None, t.ctypes.data, 7) == 1
    assert lib.ani_find_molecules(None, 0, 0, None, None, None, None, 0, None) == 1
    assert lib.ani_find_molecules_device(None, 0, 0, None, None, None, None, 0, None, None) == 1
    assert lib.ani_species_symbol(None, 0) == b""
    assert C.sizeof(C.c_int64) == 8
