"""GPU: the two restraint kernels of include/ani_md.h (ani_md_restraints_eval / ani_md_restraints_apply), through ctypes, against
the numpy form of tests/restraint_reference.py.

Cases (restraint_reference.chain_case): nr consecutive restraints of mixed kinds on a random-walk chain that crosses the faces of a
20 A box -- a lone thread, wave edges, block edges, several blocks; interior atoms collect up to four entries of the gather table,
in the hub case one atom collects eight or more; one case has a non-periodic dimension (of 1.5 A, so that folding it would show),
one takes its box from device memory while the host argument holds another.  Bars per output from
restraint_reference.evaluation_bars: ten times the reference's own rounding (float64 against np.longdouble on that case), floored at
1e-14 of the summed magnitudes of the output's terms; what is added into f and ev carries the magnitude of what was there as well.
Measured: the device stays below 0.03 of every bar.
"""
import functools

import numpy as np
import pytest

import restraint_reference as rr
from test_md_loop_kernels import Device, SENTINEL, _same

pytestmark = pytest.mark.gpu

CASES = {1: {}, 63: {}, 64: dict(pmask=3, L=(20.0, 20.0, 1.5)), 65: dict(hub=True), 255: {}, 256: {}, 257: dict(box_dev=True), 1500: {}}
WRONG_BOX = np.array([17.0, 23.0, 19.0])
STEP = 424242.0


@pytest.fixture(scope="module")
def dev():
    from lammps_ani_amd import ani_hip
    return Device(ani_hip)


@functools.lru_cache(maxsize=None)
def _case(nr):
    opt = dict(CASES[nr])
    box_dev = opt.pop("box_dev", False)
    c = rr.chain_case(nr, seed=100 + nr, **opt)
    ref, bars = rr.evaluation_bars(c["x"], c["atoms"], c["kind"], c["kappa"], c["centre"], c["len"], c["pmask"])
    rng = np.random.default_rng(nr)
    n = c["x"].shape[0]
    f0 = rng.uniform(1.0, 30.0, (n, 3)) * np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0)
    ev0 = rng.uniform(50.0, 500.0, 10) * np.where(rng.random(10) < 0.5, -1.0, 1.0)
    for a in (f0, ev0):
        a.setflags(write=False)
    return c, ref, bars, f0, ev0, box_dev


def _launch(dev, c, f0, ev0, with_virial=1, series_row=1, box_dev=False, rec=None, table=None, offset_tables=False):
    """both kernels once on fresh copies; returns the outputs on the host: cv, e, fslot, w, f, ev, rec, series [3, 1 + 2 nr].
    table: (touched, row_ptr, entries) in place of the host-built one; offset_tables: every int32 table starts one word into its
    allocation, so that it has no alignment beyond four bytes."""
    from lammps_ani_amd import ani_hip
    lib, nr, n = dev.lib, int(c["atoms"].shape[0]), int(c["x"].shape[0])
    touched, row_ptr, entries = ani_hip.restraint_gather_table(c["atoms"]) if table is None else table
    t = {k: dev.up(v) for k, v in dict(x=c["x"], atoms=c["atoms"].astype(np.int32), kind=c["kind"].astype(np.int32), kappa=c["kappa"],
                                       centre=c["centre"], touched=touched, row_ptr=row_ptr, entries=entries, f=np.array(f0), ev=np.array(ev0),
                                       rec=np.zeros(ani_hip.RESTRAINT_NREC) if rec is None else rec,
                                       series=np.full((3, 1 + 2 * nr), SENTINEL), box=c["len"]).items()}
    if offset_tables:
        for k in ("atoms", "kind", "touched", "row_ptr", "entries"):
            t[k] = dev.up(np.concatenate([[-12345], np.asarray(t[k].cpu().numpy()).reshape(-1)]).astype(np.int32))[1:]
            assert t[k].data_ptr() % 8 == 4
    out = {k: dev.up(np.full(shape, SENTINEL)) for k, shape in dict(cv=(nr,), e=(nr,), fslot=(nr, 4, 3), w=(nr, 9)).items()}
    len3 = np.array(WRONG_BOX if box_dev else c["len"], dtype=np.float64)
    rc = lib.ani_md_restraints_eval(t["x"].data_ptr(), n, t["atoms"].data_ptr(), t["kind"].data_ptr(), t["kappa"].data_ptr(),
                                    t["centre"].data_ptr(), nr, len3.ctypes.data, t["box"].data_ptr() if box_dev else None, c["pmask"],
                                    out["cv"].data_ptr(), out["e"].data_ptr(), out["fslot"].data_ptr(), out["w"].data_ptr(), None)
    assert rc == 0
    rc = lib.ani_md_restraints_apply(t["f"].data_ptr(), n, t["ev"].data_ptr(), with_virial, t["touched"].data_ptr(), t["row_ptr"].data_ptr(),
                                     t["entries"].data_ptr(), int(touched.shape[0]), out["fslot"].data_ptr(), out["cv"].data_ptr(),
                                     out["e"].data_ptr(), out["w"].data_ptr(), t["centre"].data_ptr(), t["kind"].data_ptr(), nr,
                                     t["rec"].data_ptr(), STEP, None if series_row is None else t["series"][series_row].data_ptr(), None)
    assert rc == 0
    keys = ("cv", "e", "fslot", "w")
    got = dict(zip(keys + ("f", "ev", "rec", "series"), dev.down(*[out[k] for k in keys], t["f"], t["ev"], t["rec"], t["series"])))
    _same(dev.down(t["x"])[0], c["x"], "x is not written")
    return got


def _hold(got, ref, bar, what, worst):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), ref.shape)
    err = np.abs(got - ref)
    nz = bar > 0.0
    worst[what] = float((err[nz] / bar[nz]).max()) if nz.any() else 0.0
    assert (err <= bar).all(), (what, float(err.max()), np.argwhere(err > bar)[:5].tolist(), got[err > bar][:5], ref[err > bar][:5],
                                bar[err > bar][:5])


def _case_is_what_the_recipe_says(nr):
    """faces crossed, shared atoms, nothing ill-conditioned, the special cases special; returns the touched atoms"""
    c, ref, bars, f0, ev0, box_dev = _case(nr)
    n = c["x"].shape[0]
    touched = np.unique(c["atoms"][c["atoms"] >= 0])
    counts = np.bincount(c["atoms"][c["atoms"] >= 0], minlength=n)
    assert ref["nonfinite"] == 0 and 5 <= len(c["untouched"]) <= 7 and counts[c["untouched"]].sum() == 0
    assert len(touched) == n - len(c["untouched"])
    assert counts.max() >= (8 if CASES[nr].get("hub") else min(nr, 3))
    if nr >= 63:                                                           # the wrapped chain crosses faces: without the fold it breaks
        other = rr.evaluate(c["x"], c["atoms"], c["kind"], c["kappa"], c["centre"], np.full(3, 1e6), c["pmask"])
        assert (np.abs(other["cv"] - ref["cv"]) > 1e-3).sum() >= 3
    if box_dev:
        other = rr.evaluate(c["x"], c["atoms"], c["kind"], c["kappa"], c["centre"], WRONG_BOX, c["pmask"])
        assert np.abs(other["cv"] - ref["cv"]).max() > 1e-3                # the host argument's box would give something else
    if c["pmask"] != 7:
        other = rr.evaluate(c["x"], c["atoms"], c["kind"], c["kappa"], c["centre"], c["len"], 7)
        assert np.abs(other["cv"] - ref["cv"]).max() > 1e-3                # folding the open dimension would give something else
    return touched


@pytest.mark.parametrize("nr", list(CASES))
def test_both_kernels_against_the_reference(nr, dev):
    c, ref, bars, f0, ev0, box_dev = _case(nr)
    touched = _case_is_what_the_recipe_says(nr)
    got = _launch(dev, c, f0, ev0, box_dev=box_dev)
    worst = {}
    for k in ("cv", "e", "fslot", "w"):
        _hold(got[k], ref[k], bars[k], k, worst)
    unused = c["atoms"] < 0
    assert (got["fslot"][unused] == 0.0).all()
    # f: rows of untouched atoms bitwise, the others f0 + the accumulated force
    _same(got["f"][c["untouched"]], f0[c["untouched"]], "rows of atoms in no restraint")
    _hold(got["f"][touched], (f0 + ref["facc"])[touched], (bars["facc"] + 1e-14 * np.abs(f0))[touched], "f", worst)
    assert (got["f"][touched] != f0[touched]).any(axis=1).all()
    # ev and the record
    _hold(got["ev"][0], ev0[0] + ref["E"], bars["E"] + 1e-14 * abs(ev0[0]), "ev[0]", worst)
    _hold(got["ev"][1:], ev0[1:] + ref["W"], bars["W"] + 1e-14 * np.abs(ev0[1:]), "ev[1..10)", worst)
    rec = got["rec"]
    _hold(rec[1], ref["E"], bars["E"], "record E", worst)
    _hold(rec[2:11], ref["W"], bars["W"], "record W", worst)
    _hold(rec[12], ref["max_delta"], 1e-14 * (np.abs(ref["cv"]).max() + 1.0 + np.abs(c["centre"]).max()), "record max |D|", worst)
    assert rec[0] == 1.0 and rec[11] == 0.0 and (rec[13:] == 0.0).all()
    assert got["ev"][0] == ev0[0] + rec[1] and np.array_equal(got["ev"][1:], ev0[1:] + rec[2:11])
    # the series row: only the row asked for, bitwise the kernel's own cv and e
    assert (got["series"][[0, 2]] == SENTINEL).all()
    _same(got["series"][1], np.concatenate([[STEP], got["cv"], got["e"]]), "series row")
    print(f"  nr {nr}: largest |device - reference| / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    # two launches on the same inputs are bitwise equal
    again = _launch(dev, c, f0, ev0, box_dev=box_dev)
    for k in got:
        _same(again[k], got[k], f"two launches, {k}")
    # without the virial ev[1..10) is not touched; without a row the series is not touched; the record counts on
    nov = _launch(dev, c, f0, ev0, with_virial=0, series_row=None, box_dev=box_dev, rec=rec)
    _same(nov["ev"][1:], ev0[1:], "ev[1..10) with with_virial = 0")
    assert nov["ev"][0] == got["ev"][0] and (nov["series"] == SENTINEL).all() and nov["rec"][0] == 2.0
    _same(nov["rec"][1:], rec[1:], "the record of the same evaluation")
    _same(nov["f"], got["f"], "f with with_virial = 0")
    row0 = _launch(dev, c, f0, ev0, series_row=0, box_dev=box_dev)
    assert (row0["series"][1:] == SENTINEL).all() and row0["series"][0][0] == STEP


def test_a_collinear_torsion_among_valid_restraints(dev):
    x = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [3.0, 0, 0], [1.0, 1.0, 0.0], [2.0, 1.5, 0.5], [7.0, 7.0, 7.0]])
    atoms = np.array([[0, 4, 5, 3], [0, 1, 2, 3], [0, 1, -1, -1], [4, 5, 3, -1]], dtype=np.int32)
    c = dict(x=x, atoms=atoms, kind=np.array([rr.TORSION, rr.TORSION, rr.DISTANCE, rr.ANGLE], dtype=np.int32), kappa=np.full(4, 10.0),
             centre=np.array([0.5, 0.5, 0.7, 1.0]), len=np.full(3, 50.0), pmask=7)
    ref, bars = rr.evaluation_bars(x, atoms, c["kind"], c["kappa"], c["centre"], c["len"])
    assert ref["nonfinite"] == 1 and np.isnan(ref["e"][1])
    f0, ev0 = np.full((7, 3), 3.25), np.full(10, -20.5)
    got = _launch(dev, c, f0, ev0)
    assert got["rec"][11] == 1.0 and np.isnan(got["ev"][0]) and np.isnan(got["rec"][1]) and np.isnan(got["e"][1])
    assert (got["fslot"][1] == 0.0).all() and (got["w"][1] == 0.0).all()
    ok = [0, 2, 3]
    worst = {}
    _hold(got["e"][ok], ref["e"][ok], bars["e"][ok], "e", worst)
    _hold(got["f"], f0 + ref["facc"], bars["facc"] + 1e-14 * np.abs(f0), "f", worst)
    _hold(got["ev"][1:], ev0[1:] + ref["W"], bars["W"] + 1e-14 * np.abs(ev0[1:]), "ev[1..10)", worst)
    _hold(got["rec"][12], ref["max_delta"], 1e-13, "max |D| of the finite ones", worst)
    _same(got["f"][6], f0[6], "the row of the atom in no restraint")


def test_tables_need_no_alignment_beyond_their_element_type(dev):
    c, ref, bars, f0, ev0, box_dev = _case(65)
    a, b = _launch(dev, c, f0, ev0), _launch(dev, c, f0, ev0, offset_tables=True)
    for k in a:
        _same(b[k], a[k], f"tables one word into their allocations, {k}")


def test_a_gather_table_that_points_outside_is_skipped_and_counted(dev):
    """one touched word outside [0, natoms) and two entries outside [0, 4 nr): nothing is followed, the three words are counted in
    record [13] and E is NaN; every other atom gets exactly what the good table gives it"""
    from lammps_ani_amd import ani_hip
    c, ref, bars, f0, ev0, box_dev = _case(65)
    n, nr = c["x"].shape[0], c["atoms"].shape[0]
    good = _launch(dev, c, f0, ev0)
    touched, row_ptr, entries = (a.copy() for a in ani_hip.restraint_gather_table(c["atoms"]))
    lost = int(touched[3])
    touched[3] = n                                                        # this atom's whole row is dropped
    qa, qb = int(row_ptr[10]), int(row_ptr[20])                           # the first entries of two other atoms
    ea, eb = int(entries[qa]), int(entries[qb])
    entries[qa], entries[qb] = 4 * nr, -1
    got = _launch(dev, c, f0, ev0, table=(touched, row_ptr, entries))
    assert got["rec"][13] == 3.0 and np.isnan(got["rec"][1]) and np.isnan(got["ev"][0]) and good["rec"][13] == 0.0
    _same(got["rec"][2:13], good["rec"][2:13], "W, the non-finite count and max |D| do not depend on the gather table")
    _same(got["ev"][1:], good["ev"][1:], "ev[1..10)")
    hit = [lost, int(touched[10]), int(touched[20])]
    rest = np.setdiff1d(np.arange(n), hit)
    _same(got["f"][rest], good["f"][rest], "rows of the atoms whose words are good")
    _same(got["f"][lost], f0[lost], "the row of the atom whose touched word points outside")
    for atom, word in ((hit[1], ea), (hit[2], eb)):
        words = [int(w) for w in entries[row_ptr[list(touched).index(atom)]: row_ptr[list(touched).index(atom) + 1]] if 0 <= w < 4 * nr]
        assert word not in words
        acc = np.zeros(3)
        for w in words:
            acc = acc + good["fslot"].reshape(-1, 3)[w]
        _same(got["f"][atom], f0[atom] + acc, "the row of an atom with one entry skipped")


def test_nothing_is_launched_without_restraints(dev):
    lib = dev.lib
    assert lib.ani_md_restraints_eval(None, 0, None, None, None, None, 0, None, None, 7, None, None, None, None, None) == 0
    assert lib.ani_md_restraints_apply(None, 0, None, 1, None, None, None, 0, None, None, None, None, None, None, 0, None, 0.0, None, None) == 0
