"""GPU: the molecule finder (ani_set_bond_table / ani_find_molecules* of include/ani_hip.h, kernels in ani_kernels_mol.hip) against
the CPU reference tests/molecule_reference.py.  The results are integers: every comparison is an equality.

The table is the reactive workloads' analysis table (tests/golden/bond_table_analysis.json).  Before the GPU runs, every test
asserts on the CPU that no candidate pair lies within 1e-6 A of its threshold, so that the fp64 arithmetic of the two sides cannot
disagree about a bond."""
import ctypes as C

import numpy as np
import pytest

import molecule_reference as mr
from lammps_ani_amd import harness as hx

pytestmark = pytest.mark.gpu

TABLE = mr.load_table()
S = 7
SENT = -77
GAP = 1e-6
ANI_ERR_ARG, ANI_ERR_CAPACITY = 1, 4


@pytest.fixture(scope="module")
def hip():
    from lammps_ani_amd import ani_hip
    return ani_hip


class Case:
    """an input, its owners and the reference's answer (computed once per module, never changed)"""

    def __init__(self, inp, owner, table=TABLE):
        self.inp, self.owner, self.table = inp, owner, table
        assert mr.threshold_gap(inp, table) > GAP
        self.labels, self.formulas, self.summary, self.image_bonds = mr.find_molecules(inp, table, owner)
        self.rows = mr.formula_rows(self.formulas)
        for a in (self.labels, self.summary, self.rows):
            a.setflags(write=False)


_cases = {}


def case(name):
    if name in _cases:
        return _cases[name]
    if name == "random":          # deep trees, many bonds through an image
        inp = hx.decompose(hx.random_box(600, 4, 16.0, seed=7))
        c = Case(inp, mr.owners_of(inp))
        assert c.summary.tolist() == [179, 50, 0, 994, 92, 0] and c.image_bonds == 102
    elif name == "random_all_foreign":
        c = Case(case("random").inp, None)
        assert c.summary[2] > 0
    elif name == "combustion":    # CH4 + 2 O2, translated until molecules straddle the faces
        sysm = hx.combustion_box(1152, seed=3)
        L = sysm.boxhi - sysm.boxlo
        a = L / int(np.ceil((3 * (1152 // 9)) ** (1.0 / 3.0)))   # lattice spacing of the molecules' centres
        x = sysm.boxlo + np.mod(sysm.x + 0.5 * a - sysm.boxlo, L)
        shifted = hx.System(x, sysm.types, sysm.boxlo, sysm.boxhi)
        inp = hx.decompose(shifted)
        c = Case(inp, mr.owners_of(inp))
        c.sysm = shifted
        assert c.image_bonds >= 20
        assert c.summary.tolist() == [384, 2, 0, 1536, 5, 0]
    elif name == "two_ranks":     # rank 0 of 2: the other rank's ghosts are foreign
        inp = hx.decompose(hx.random_box(600, 4, 16.0, seed=7), grid=(2, 1, 1), rank=0)
        c = Case(inp, mr.owners_of(inp, 0))
        assert c.summary[2] > 0 and c.summary[5] > 0 and (c.owner >= 0).any() and (c.owner < 0).any()
    else:
        raise KeyError(name)
    _cases[name] = c
    return c


def make(hip, model_cache, table=TABLE, **kw):
    ani = hip.ANI(model_cache("ani2x", 1, 11), 0, **kw)
    if table is not None:
        ani.set_bond_table(table)
    return ani


def raw_find(ani, x, nlocal, owner, cap, pad=3):
    """the host entry through ctypes with sentinels behind every output: (rc, labels, the rows written, summary)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    own = None if owner is None else np.ascontiguousarray(owner, dtype=np.int64)
    mol = np.full(nlocal + pad, SENT, dtype=np.int32)
    rows = np.full((cap + pad, S + 1), SENT, dtype=np.int32)
    summ = np.full(6 + pad, SENT, dtype=np.int64)
    rc = ani._lib.ani_find_molecules(ani._h, x.shape[0], nlocal, x.ctypes.data, None if own is None else own.ctypes.data,
                                     mol.ctypes.data, rows.ctypes.data, cap, summ.ctypes.data)
    assert (mol[nlocal:] == SENT).all() and (rows[cap:] == SENT).all() and (summ[6:] == SENT).all()
    n = int(min(summ[1], cap))
    assert (rows[n:] == SENT).all()
    return rc, mol[:nlocal], rows[:n], summ[:6]


def check(ani, hip, c, owner="case"):
    owner = c.owner if owner == "case" else owner
    rc, mol, rows, summ = raw_find(ani, c.inp.x, c.inp.nlocal, owner, 64)
    print("summary", summ.tolist(), "reference", c.summary.tolist())
    assert rc == 0, ani._lib.ani_last_error(ani._h)
    assert np.array_equal(summ, c.summary)
    assert np.array_equal(mol, c.labels)
    assert np.array_equal(rows, c.rows)
    sym = ani.species_symbols()
    assert sym == list(mr.SYMBOLS_ANI2X)
    want = {}
    for comp, n in c.formulas.items():
        want[hip.formula_string(comp, sym)] = n
    mol2, fdict, summ2 = ani.find_molecules(c.inp, owner=owner)
    assert np.array_equal(mol2, c.labels) and fdict == want and np.array_equal(summ2, c.summary)
    return mol, rows, summ


def test_random_box_callers_list(model_cache, hip):
    """case 1: one rank, periodic, the caller's list installed by a step (dense segments)"""
    c = case("random")
    assert c.inp.nghost == 3404 and c.inp.numneigh.max() == 244
    ani = make(hip, model_cache)
    ani.compute(c.inp, ago=0)
    check(ani, hip, c)
    check(ani, hip, case("random_all_foreign"), owner=None)   # no owners given, no fold installed: every ghost is foreign
    ani.close()


def _list_layout(ani, nlocal):
    pn, po, pj = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert ani._lib.ani_debug_list(ani._h, C.byref(pn), C.byref(po), C.byref(pj)) == 0
    nn = ani.debug_read(pn, (nlocal,), np.int32)
    off = ani.debug_read(po, (nlocal + 1,), np.int32)
    return "dense" if np.array_equal(np.diff(off), nn) else "rows"


def test_random_box_built_lists_and_repeats(model_cache, hip):
    """case 2: the library's own list, in both of its layouts; five calls on one handle give the same canonical answer"""
    c = case("random")
    ani = make(hip, model_cache)
    layouts = []
    for _ in range(3):
        assert ani.build_list(c.inp.species, c.inp.x, c.inp.nlocal, 7.1) == c.inp.npairs
        layouts.append(_list_layout(ani, c.inp.nlocal))
        first = check(ani, hip, c)
        for _ in range(4):
            again = raw_find(ani, c.inp.x, c.inp.nlocal, c.owner, 64)
            assert again[0] == 0 and all(np.array_equal(p, q) for p, q in zip(first, again[1:]))
    print("layouts", layouts)
    assert "rows" in layouts and "dense" in layouts
    ani.close()


def _combustion(ani, hip, c, fold):
    import torch
    ani.compute(c.inp, ago=0)
    assert c.formulas == {(4, 1, 0, 0, 0, 0, 0): 128, (0, 0, 0, 2, 0, 0, 0): 256}
    check(ani, hip, c)
    mol, fdict, _ = ani.find_molecules(c.inp, owner=c.owner)
    assert fdict == {"CH4": 128, "O2": 256} and np.array_equal(mol, c.labels)
    if fold:
        dev = torch.device("cuda:0")
        L = c.sysm.boxhi - c.sysm.boxlo
        d_owner = torch.as_tensor(c.owner, device=dev)
        d_shift = torch.as_tensor(c.inp.shift * L, dtype=torch.float64, device=dev).contiguous()
        assert np.abs(c.inp.x[c.inp.nlocal:] - (c.inp.x[c.owner] + c.inp.shift * L)).max() < 1e-9
        ani.set_ghost_fold(d_owner.data_ptr(), d_shift.data_ptr(), c.inp.nghost)
        check(ani, hip, c, owner=None)   # the owners come from the fold
        mol, fdict, _ = ani.find_molecules(c.inp)
        assert fdict == {"CH4": 128, "O2": 256} and np.array_equal(mol, c.labels)
        torch.cuda.synchronize()


def test_combustion_box_owner_and_fold(model_cache, hip):
    """case 3: molecules across the periodic faces, owners passed and owners from an installed ghost fold"""
    ani = make(hip, model_cache)
    _combustion(ani, hip, case("combustion"), fold=True)
    ani.close()


def test_combustion_box_fp64_handle(model_cache, hip):
    """case 8: the finder does not depend on the handle's precision"""
    ani = make(hip, model_cache, use_single=False)
    _combustion(ani, hip, case("combustion"), fold=False)
    ani.close()


def test_open_molecules_of_one_rank_of_two(model_cache, hip):
    """case 4"""
    c = case("two_ranks")
    ani = make(hip, model_cache)
    ani.compute(c.inp, ago=0)
    check(ani, hip, c)
    ani.close()


def test_formula_capacity(model_cache, hip):
    """case 5: formula_cap = 2 -- ANI_ERR_CAPACITY from the host entry, the full number in summary[1], nothing past two rows from
    either entry (the device entry writes into a caller's array: the sentinels sit in device memory there)"""
    import torch
    c = case("random")
    ani = make(hip, model_cache)
    ani.compute(c.inp, ago=0)
    rc, mol, rows, summ = raw_find(ani, c.inp.x, c.inp.nlocal, c.owner, 2)
    assert rc == ANI_ERR_CAPACITY and b"formula_cap" in ani._lib.ani_last_error(ani._h)
    assert np.array_equal(summ, c.summary) and summ[1] == 50 and np.array_equal(mol, c.labels)
    known = {tuple(r) for r in c.rows.tolist()}
    assert rows.shape == (2, S + 1) and tuple(rows[0]) in known and tuple(rows[1]) in known
    assert tuple(rows[0][:S]) < tuple(rows[1][:S])
    with pytest.raises(hip.AniError, match="formula_cap"):
        ani.find_molecules(c.inp, owner=c.owner, formula_cap=2)
    dev = torch.device("cuda:0")
    d_x = torch.as_tensor(c.inp.x, dtype=torch.float64, device=dev).contiguous()
    d_owner = torch.as_tensor(c.owner, device=dev)
    for cap in (2, 0, 50):
        d_rows = torch.full((cap + 3, S + 1), SENT, dtype=torch.int32, device=dev)
        d_mol = torch.full((c.inp.nlocal + 3,), SENT, dtype=torch.int32, device=dev)
        d_sum = torch.full((9,), SENT, dtype=torch.int64, device=dev)
        ani.find_molecules_device(c.inp.ntotal, c.inp.nlocal, d_x.data_ptr(), d_owner.data_ptr(), d_mol.data_ptr(), d_rows.data_ptr(), cap,
                                  d_sum.data_ptr())
        torch.cuda.synchronize()
        r, m, s = d_rows.cpu().numpy(), d_mol.cpu().numpy(), d_sum.cpu().numpy()
        assert (r[cap:] == SENT).all() and (m[c.inp.nlocal:] == SENT).all() and (s[6:] == SENT).all()
        assert np.array_equal(s[:6], c.summary) and np.array_equal(m[: c.inp.nlocal], c.labels)
        assert {tuple(q) for q in r[:cap].tolist()} <= known and len({tuple(q) for q in r[:cap].tolist()}) == cap
    # outputs left out
    ani.find_molecules_device(c.inp.ntotal, c.inp.nlocal, d_x.data_ptr(), d_owner.data_ptr(), None, None, 0, None)
    torch.cuda.synchronize()
    ani.close()


def _chains(lengths, seed=5):
    """carbon chains along x, 1.0 A between neighbours, 20 A apart in y, atoms in a shuffled order; open box, no ghosts"""
    pts = []
    for k, n in enumerate(lengths):
        p = np.zeros((n, 3))
        p[:, 0] = np.arange(n) * 1.0
        p[:, 1] = 20.0 * k
        pts.append(p)
    x = np.concatenate(pts)
    x = x[np.random.default_rng(seed).permutation(len(x))]
    lo, hi = x.min(0) - 10.0, x.max(0) + 10.0
    sysm = hx.System(x, np.full(len(x), 2, dtype=np.int32), lo, hi, periodic=(False, False, False))
    inp = hx.decompose(sysm)
    assert inp.nghost == 0 and inp.nlocal == len(x)
    table = np.zeros((S, S))
    table[1, 1] = 1.2
    return Case(inp, None, table)


@pytest.mark.parametrize("lengths", [(600,), (600, 520, 600, 3)])
def test_molecule_too_large_for_its_key_field(lengths, model_cache, hip):
    """case 6: seven species leave 9 bits per species in the key (counts below 511): a chain of 600 bonded atoms takes the path of
    the molecules listed by root, and its 599 bonds in a shuffled atom order make the deepest trees the union sees.  Several such
    molecules: those of one composition make one row."""
    c = _chains(lengths)
    if lengths == (600,):
        assert c.rows.tolist() == [[0, 600, 0, 0, 0, 0, 0, 1]] and c.summary.tolist() == [1, 1, 0, 1198, 600, 0] and (c.labels == 0).all()
    else:
        assert c.rows.tolist() == [[0, 3, 0, 0, 0, 0, 0, 1], [0, 520, 0, 0, 0, 0, 0, 1], [0, 600, 0, 0, 0, 0, 0, 2]]
    ani = make(hip, model_cache, table=c.table)
    ani.build_list(c.inp.species, c.inp.x, c.inp.nlocal, 7.1)
    _, rows, _ = check(ani, hip, c)
    _, fdict, _ = ani.find_molecules(c.inp)
    assert fdict == ({"C600": 1} if lengths == (600,) else {"C3": 1, "C520": 1, "C600": 2})
    ani.close()


def test_refusals(model_cache, hip):
    """case 7: each refusal is ANI_ERR_ARG with a message that names the reason, and the handle's next step is what it was"""
    c = case("random")
    ani = make(hip, model_cache, table=None)
    lib, h = ani._lib, ani._h
    x = np.ascontiguousarray(c.inp.x)
    summ = np.zeros(6, dtype=np.int64)

    def find(a=ani, nt=c.inp.ntotal, nl=c.inp.nlocal):
        rc = a._lib.ani_find_molecules(a._h, nt, nl, x.ctypes.data, None, None, None, 0, summ.ctypes.data)
        return rc, a._lib.ani_last_error(a._h).decode()

    def set_table(t, n=S):
        t = np.ascontiguousarray(t, dtype=np.float64)
        return lib.ani_set_bond_table(h, t.ctypes.data, n), lib.ani_last_error(h).decode()

    ani.set_bond_table(TABLE)
    rc, msg = find()
    assert rc == ANI_ERR_ARG and "no neighbour list" in msg
    before = ani.compute(c.inp, ago=0)
    ani.set_bond_table(None)
    rc, msg = find()
    assert rc == ANI_ERR_ARG and "no bond table" in msg
    rc, msg = set_table(TABLE[:4, :4], 4)
    assert rc == ANI_ERR_ARG and "nspecies" in msg and "7" in msg
    t = TABLE.copy()
    t[0, 3] = 3.6   # ANI-2x: Rca = 3.5 A, Rcr = 5.1 A
    t[3, 0] = 3.6
    rc, msg = set_table(t)
    assert rc == ANI_ERR_ARG and "cutoff" in msg and "[H][O]" in msg
    t = TABLE.copy()
    t[1, 2] += 0.01
    rc, msg = set_table(t)
    assert rc == ANI_ERR_ARG and "asymmetric" in msg
    rc, msg = find()
    assert rc == ANI_ERR_ARG and "no bond table" in msg   # a refused table is not installed
    ani.set_bond_table(TABLE)
    rc, msg = find(nt=c.inp.ntotal - 1)
    assert rc == ANI_ERR_ARG and "differ" in msg
    rc, msg = find(nl=c.inp.nlocal - 1)
    assert rc == ANI_ERR_ARG and "differ" in msg
    with pytest.raises(hip.AniError, match="no species"):
        ani.set_bond_table({("H", "Xe"): 1.0})
    ani.set_bond_table({("H", "O"): 1.16, ("O", "O"): 1.68})
    ani.set_bond_table(TABLE)
    assert find()[0] == 0 and np.array_equal(summ, case("random_all_foreign").summary)
    after = ani.compute(c.inp, ago=1)
    # the same list and positions: the two steps differ by the order of the fp32 force atomics only (the bar of
    # tests/test_md_device.py for two evaluations of one configuration)
    assert abs(after["energy"] - before["energy"]) < 1e-3 and np.abs(after["force"] - before["force"]).max() < 1e-3
    ani.close()
    # a half-list handle
    half = hx.decompose(hx.random_box(600, 4, 16.0, seed=7), half=True)
    ani = make(hip, model_cache, use_fullnbr=False)
    ani.compute(half, ago=0)
    rc, msg = find(ani, half.ntotal, half.nlocal)
    assert rc == ANI_ERR_ARG and "half" in msg
    ani.close()


def test_verlet_run_find_molecules(model_cache, hip):
    """case 9: the loop's own positions, list and owner maps, after 20 steps with a re-neighbouring among them"""
    import torch
    from lammps_ani_amd import md
    sysm = case("combustion").sysm
    inp = hx.decompose(sysm)
    ani = make(hip, model_cache)
    run = md.VerletRun(ani, inp, sysm.boxhi - sysm.boxlo, torch.device("cuda:0"), dt=0.1, box_lo=sysm.boxlo)
    run.create_velocities(300.0)
    nb = run.nbuilds
    for k in range(20):
        run.step(force_rebuild=(k == 12))
    assert run.nbuilds == nb + 1
    mol, fdict, summ = run.find_molecules()
    n = run.nlocal
    x = run.x[:n].cpu().numpy()
    assert np.abs(x - inp.x[:n]).max() > 1e-3   # they moved
    L = sysm.boxhi - sysm.boxlo
    now = hx.decompose(hx.System(sysm.boxlo + np.mod(x - sysm.boxlo, L), sysm.types, sysm.boxlo, sysm.boxhi))
    assert np.array_equal(now.tag[:n], np.arange(n))
    ref = Case(now, mr.owners_of(now))
    print("summary", summ.tolist(), "reference", ref.summary.tolist(), "image bonds", ref.image_bonds)
    assert ref.image_bonds > 0
    assert np.array_equal(summ, ref.summary) and np.array_equal(mol, ref.labels)
    assert fdict == {hip.formula_string(comp, ani.species_symbols()): k for comp, k in ref.formulas.items()}
    # the ghost rows of the loop's positions are the images of the owned rows
    xg = run.x.cpu().numpy()
    own, sh = run.dc.send_idx.cpu().numpy(), run.dc.send_shift.cpu().numpy()
    assert np.abs(xg[n:] - (xg[own] + sh)).max() < 1e-9
    run.step()
    assert np.isfinite(run.potential_energy())   # the loop goes on
    ani.close()
