"""No GPU: the list forms of tests/list_forms.py on the fp64 oracle, and the structural conditions of the shared inputs.

a. The oracle walks ilist itself (oracle/ani_oracle.c), so ``Oracle.compute(form(inp))`` must equal ``expected(Oracle.compute(inp),
   perm)`` to fp64 summation-order noise: the project's fp64 bars (tests/test_hip_parity.py,
   test_hip_double_precision_matches_golden): force 1e-8, eatom 1e-7, virial 1e-6, energy 9e-9 relative.  This validates the helper
   and lets tests/test_list_contract.py reuse one oracle result per input across forms.
b. The forms discriminate: an eatom array returned in atom order instead of ilist order differs from the expected one by far more
   than the fp32 parity bar, and no permutation leaves a long run of centres in place.
c. The inputs still reach the edges they were made for.
"""
import numpy as np
import pytest

import list_forms as lf
from lammps_ani_amd import model_file as mf

E_TOL = 2e-3   # the fp32 per-centre energy bar of tests/test_hip_parity.py


@pytest.fixture(scope="module")
def oracle_ref(model_cache):
    """input id -> oracle result of the identity form (computed once)"""
    from oracle import Oracle
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Oracle(lf.model_path(name, model_cache)).compute(lf.build_input(name))
        return cache[name]

    return get


@pytest.mark.parametrize("form", lf.FORMS)
@pytest.mark.parametrize("name", lf.INPUT_IDS)
def test_oracle_is_invariant_under_the_forms(name, form, model_cache, oracle_ref):
    from oracle import Oracle
    inp = lf.build_input(name)
    got_inp, perm = lf.apply_form(inp, form)
    assert np.array_equal(np.sort(got_inp.jlist), np.sort(inp.jlist)) and int(got_inp.numneigh.sum()) == inp.npairs
    got = Oracle(lf.model_path(name, model_cache)).compute(got_inp)
    ref = lf.expected(oracle_ref(name), perm)
    de = abs(got["energy"] - ref["energy"])
    df = np.abs(got["force"] - ref["force"]).max()
    dea = np.abs(got["eatom"] - ref["eatom"]).max()
    dv = np.abs(got["virial"] - ref["virial"]).max()
    print(f"{name}/{form}: |dE|={de:.2e} (|E|={abs(ref['energy']):.2e}) max|dF|={df:.2e} max|dEatom|={dea:.2e} max|dV|={dv:.2e}")
    assert de < 9e-9 * abs(ref["energy"])
    assert df < 1e-8
    assert dea < 1e-7
    assert dv < 1e-6


@pytest.mark.parametrize("form", lf.FORMS)
@pytest.mark.parametrize("name", lf.INPUT_IDS)
def test_forms_discriminate(name, form, oracle_ref):
    """eatom by atom instead of by centre would miss the expected array by the difference of two self energies"""
    inp = lf.build_input(name)
    perm = lf.form_perm(form, inp.nlocal)
    ref = oracle_ref(name)
    gap = np.abs(ref["eatom"] - ref["eatom"][perm]).max()
    print(f"{name}/{form}: max|eatom - eatom[perm]| = {gap:.3e}, longest fixed run {lf.longest_fixed_run(perm)}")
    assert gap > 1000 * E_TOL
    assert lf.longest_fixed_run(perm) <= 8


def test_reorder_and_shuffle_keep_every_centres_neighbour_set():
    inp = lf.build_input("tiny_generic")
    base = {int(i): np.sort(s) for i, s in zip(inp.ilist, lf.segments(inp))}
    for form in lf.FORMS:
        got, perm = lf.apply_form(inp, form)
        assert np.array_equal(got.ilist, inp.ilist[perm]) and np.array_equal(got.numneigh, inp.numneigh[perm])
        segs = lf.segments(got)
        for k, i in enumerate(got.ilist.tolist()):
            assert np.array_equal(np.sort(segs[k]), base[i])
            if form != "random+shuffled":
                assert np.array_equal(segs[k], lf.segments(inp)[perm[k]])
    shuffled = lf.apply_form(inp, "random+shuffled")[0]
    unshuffled = lf.apply_form(inp, "random")[0]
    assert not np.array_equal(shuffled.jlist, unshuffled.jlist)


def test_expected_moves_only_what_is_indexed_by_centre():
    n = 6
    perm = np.array([3, 0, 5, 1, 4, 2])
    ref = dict(energy=1.0, force=np.arange(3.0 * n).reshape(n, 3), eatom=np.arange(float(n)), virial=np.eye(3), aev=None, gaev=None,
               atom_virial=np.arange(9.0 * n).reshape(n, 9),
               deviation=dict(member_energy=np.arange(2.0), atom_energy_dev=10 + np.arange(float(n)), member_dforce=np.zeros((n, 2, 3)),
                              atom_force_dev=20 + np.arange(float(n)), summary=np.arange(4.0)))
    out = lf.expected(ref, perm)
    assert np.array_equal(out["eatom"], perm.astype(float)) and np.array_equal(out["deviation"]["atom_energy_dev"], 10.0 + perm)
    for k in ("force", "virial", "atom_virial"):
        assert out[k] is ref[k]
    for k in ("member_energy", "member_dforce", "atom_force_dev", "summary"):
        assert out["deviation"][k] is ref["deviation"][k]
    assert out["energy"] == 1.0


# ---- c. structural conditions -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", lf.INPUT_IDS)
def test_inputs_stay_inside_the_kernels_capacities(name, model_cache):
    """no capacity overflow is provoked: lists shorter than 256 entries, fewer than 96 neighbours inside Rca"""
    inp = lf.build_input(name)
    m = mf.read_model(lf.model_path(name, model_cache))
    assert np.array_equal(inp.ilist, np.arange(inp.nlocal))
    assert int(inp.numneigh.max()) < 256
    assert int(lf.neighbours_within(inp, m.Rca).max()) < 96
    print(f"{name}: nlocal {inp.nlocal} ntotal {inp.ntotal} max numneigh {int(inp.numneigh.max())} "
          f"max inside Rca {int(lf.neighbours_within(inp, m.Rca).max())}")


@pytest.mark.parametrize("name", list(lf.CHUNK_NLOCAL))
def test_chunk_boxes_sit_on_the_chunk_edges(name):
    inp = lf.build_input(name)
    assert inp.nlocal == lf.CHUNK_NLOCAL[name]
    assert inp.nlocal in (4096, 4096 + 1, 2 * 4096 + 1)
    assert int(inp.numneigh.max()) > 128   # the longest compaction kernel (more than two waves' worth of candidates)


def test_cluster_has_empty_rows_between_dense_ones():
    inp = lf.build_input("cluster_isolated")
    _, isolated = lf.cluster_system()
    assert inp.nghost == 0 and inp.ntotal == inp.nlocal == 500 + lf.N_ISOLATED
    empty = np.flatnonzero(inp.numneigh == 0)
    assert len(empty) >= 5 and set(isolated.tolist()) <= set(empty.tolist())
    # between dense ones: centres with neighbours on both sides of the first, and behind the last dense centre at the end
    assert inp.numneigh[empty[0] - 1] > 0 and inp.numneigh[empty[0] + 1] > 0 and empty[-1] == inp.nlocal - 1


def test_ghost_only_species_is_only_among_the_ghosts(model_cache):
    inp = lf.build_input("ghost_only_species")
    m = mf.read_model(lf.model_path("ghost_only_species", model_cache))
    t = lf.GHOST_ONLY_TYPE
    assert int((inp.types[: inp.nlocal] == t).sum()) == 0
    assert int((inp.types[inp.nlocal:] == t).sum()) > 0
    i = np.repeat(inp.ilist.astype(np.int64), inp.numneigh)
    j = inp.jlist.astype(np.int64)
    d = inp.x[j] - inp.x[i]
    close = (inp.types[j] == t) & (np.einsum("ij,ij->i", d, d) < m.Rca ** 2)
    print(f"ghost_only_species: {inp.nlocal} centres, {int((inp.types[inp.nlocal:] == t).sum())} ghosts of the species, "
          f"{int(close.sum())} entries of them inside Rca")
    assert int(close.sum()) >= 1
    assert np.all(j[close] >= inp.nlocal)
    # every other species of the model has local centres: exactly one bucket is empty
    assert set(np.unique(inp.types[: inp.nlocal]).tolist()) == {1, 2, 4}
