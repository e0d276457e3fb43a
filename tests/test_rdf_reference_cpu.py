"""CPU: the numpy reference of the RDF accumulators (tests/rdf_reference.py) against a plain Python loop and against itself, the
identities of ani_hip.rdf_normalise, and the pins of the cases tests/test_rdf.py runs on the GPU: each lies at least 1e-9 A from
every bin edge (so the fp64 arithmetic of the two sides cannot disagree about a bin), and its totals per pair are written down."""
import itertools

import numpy as np
import pytest

import rdf_reference as rr
from lammps_ani_amd import harness as hx

GAP = 1e-9


def test_reference_equals_a_plain_triple_loop():
    sysm = hx.random_box(40, 3, 8.0, seed=3)
    pairs, nbins, rmax = [(0, 0), (0, 1), (1, 0), (2, 1), (2, 2)], 17, 5.1
    L = sysm.boxhi - sysm.boxlo
    sp = sysm.types - 1
    inv_dr = nbins / rmax
    want = np.zeros((len(pairs), nbins), dtype=np.uint64)
    for i in range(sysm.natoms):
        for j in range(sysm.natoms):
            for sh in itertools.product((-1, 0, 1), repeat=3):
                if i == j and sh == (0, 0, 0):
                    continue
                if (sp[i], sp[j]) not in pairs:
                    continue
                dx, dy, dz = (sysm.x[j] + np.array(sh) * L) - sysm.x[i]
                r = float(np.sqrt(dx * dx + dy * dy + dz * dz))
                if r < rmax and int(r * inv_dr) < nbins:
                    want[pairs.index((sp[i], sp[j])), int(r * inv_dr)] += 1
    got, centres = rr.counts(sysm, pairs, nbins, rmax)
    assert want.sum() > 500
    assert np.array_equal(got, want)
    assert centres.tolist() == [int((sp == a).sum()) for a, _ in pairs]
    # the same through the decomposed input (images as ghosts)
    got2, centres2 = rr.counts(hx.decompose(sysm), pairs, nbins, rmax)
    assert np.array_equal(got2, want) and np.array_equal(centres2, centres)


def test_ordered_pairs_mirror_each_other_on_a_whole_box():
    c = rr.case("random_whole")
    slot = {tuple(p): k for k, p in enumerate(c.pairs.tolist())}
    for (a, b), k in slot.items():
        assert np.array_equal(c.counts[k], c.counts[slot[(b, a)]])
    assert np.array_equal(c.counts, rr.case("random").counts) and np.array_equal(c.centres, rr.case("random").centres)


def test_ranks_add_up_to_the_whole_box():
    whole, r0, r1 = rr.case("random_whole"), rr.case("rank0"), rr.case("rank1")
    assert r0.obj.nlocal + r1.obj.nlocal == 600 and r0.obj.nlocal > 0 and r1.obj.nlocal > 0
    assert np.array_equal(r0.counts + r1.counts, whole.counts)
    assert np.array_equal(r0.centres + r1.centres, whole.centres)


def test_gpu_cases_are_pinned():
    """gaps and totals of the cases of tests/test_rdf.py"""
    total16 = [2730, 2658, 2871, 3165, 2658, 2704, 2839, 3241, 2871, 2839, 3074, 3365, 3165, 3241, 3365, 3850]
    c = rr.case("random")
    assert c.obj.nlocal == 600 and c.obj.nghost == 3404
    assert c.gap > 1e-6 > GAP and c.totals == total16
    assert c.centres.tolist() == [139] * 4 + [143] * 4 + [150] * 4 + [168] * 4
    c = rr.case("random_4096")
    assert c.gap > 4e-8 > GAP and c.totals == total16
    c = rr.case("random_subset")
    assert c.gap > 2e-5 > GAP and c.totals == [161, 149, 188] and c.centres.tolist() == [139, 139, 150]
    c = rr.case("rank0")
    assert (c.obj.nlocal, c.obj.nghost) == (297, 2674) and c.gap > 1e-6
    assert c.totals == [1415, 1312, 1522, 1552, 1358, 1362, 1474, 1607, 1437, 1388, 1532, 1609, 1490, 1494, 1590, 1759]
    c = rr.case("rank1")
    assert (c.obj.nlocal, c.obj.nghost) == (303, 2653) and c.gap > 1e-6
    assert c.totals == [1315, 1346, 1349, 1613, 1300, 1342, 1365, 1634, 1434, 1451, 1542, 1756, 1675, 1747, 1775, 2091]
    c = rr.case("one_atom")
    assert (c.obj.nlocal, c.obj.nghost) == (1, 124) and c.gap > 1e-2 and c.totals == [6] and c.centres.tolist() == [1]
    # its six neighbours are its own images along the axes, 4 A away: bin (int)(4 * 64 / 5.1) = 50
    assert int(c.counts[0, 50]) == 6
    whole = rr.counts(rr.one_atom_system(), [(3, 3)], 64, rr.RCR)
    assert np.array_equal(whole[0], c.counts)


def test_edge_gap_sees_a_pair_on_an_edge():
    x = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 3.0], [4.0, 1.0, 1.0]])
    sysm = hx.System(x, np.array([1, 1, 1], dtype=np.int32), np.zeros(3), np.full(3, 40.0))
    assert rr.edge_gap(sysm, [(0, 0)], 4, 4.0) == 0.0          # r = 2 and r = 3 are edges
    assert abs(rr.edge_gap(sysm, [(0, 0)], 4, 4.4) - 0.2) < 1e-12   # r = 2 against the edge 2.2
    # a pair just beyond rmax is "nearly counted": r = 3 against rmax = 2.9999
    assert abs(rr.edge_gap(sysm, [(0, 0)], 1, 2.9999) - 1e-4) < 1e-12


def _normalise():
    from lammps_ani_amd import ani_hip
    return ani_hip.rdf_normalise


def test_rdf_normalise_identities():
    norm = _normalise()
    c = rr.case("random_whole")
    n_of = np.bincount(c.obj.types - 1, minlength=7)
    vol = float(np.prod(c.obj.boxhi - c.obj.boxlo))
    frames = 3
    out = norm(c.counts * np.uint64(frames), c.centres * np.uint64(frames), c.nbins, c.rmax, c.pairs, n_of, vol)
    assert out["r"].shape == (c.nbins,) and out["g"].shape == out["coord"].shape == c.counts.shape
    dr = c.rmax / c.nbins
    assert np.allclose(out["r"], (np.arange(c.nbins) + 0.5) * dr, rtol=0, atol=1e-14)
    edges = np.arange(c.nbins + 1) * dr
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    for p, (a, b) in enumerate(c.pairs.tolist()):
        total = float(c.counts[p].sum()) * frames
        cen = float(c.centres[p]) * frames
        assert out["coord"][p, -1] * cen == pytest.approx(total, rel=1e-14)
        rho_b = (n_of[b] - (1 if a == b else 0)) / vol
        assert (out["g"][p] * rho_b * shell).sum() == pytest.approx(out["coord"][p, -1], rel=1e-12)
    # frames do not change a normalised function
    one = norm(c.counts, c.centres, c.nbins, c.rmax, c.pairs, n_of, vol)
    assert np.allclose(one["g"], out["g"], rtol=1e-14, atol=0) and np.allclose(one["coord"], out["coord"], rtol=1e-14, atol=0)
    # an ideal gas has g = 1: counts set to the expected number per shell
    ideal = np.outer(c.centres.astype(np.float64), shell) * ((n_of[c.pairs[:, 1]] - (c.pairs[:, 0] == c.pairs[:, 1])) / vol)[:, None]
    assert np.allclose(norm(ideal, c.centres, c.nbins, c.rmax, c.pairs, n_of, vol)["g"], 1.0, rtol=1e-12, atol=0)


def test_rdf_normalise_gives_zeros_for_an_absent_species():
    norm = _normalise()
    pairs = [(0, 0), (0, 5), (5, 0), (4, 4)]
    counts = np.zeros((4, 8), dtype=np.uint64)
    counts[0] = 3
    counts[3] = 2     # a lone atom of species 4 seeing its own images: N_b - 1 = 0
    centres = np.array([10, 10, 0, 1], dtype=np.uint64)
    out = norm(counts, centres, 8, 4.0, pairs, [10, 0, 0, 0, 1, 0, 0], 1000.0)
    for k in ("r", "g", "coord"):
        assert np.isfinite(out[k]).all()
    assert (out["g"][0] > 0).all() and (out["g"][1:] == 0).all()
    assert (out["coord"][1:3] == 0).all() and out["coord"][3, -1] == 16.0
