"""CPU reference of the RDF accumulators (ani_rdf_*, include/ani_hip.h), written from the definitions there and not from the
library: brute force in numpy, no neighbour list.

  centre   an owned atom
  count    ordered pair (centre i, atom or image j != i) of a configured species pair p = (s_i, s_j) with
           r = sqrt(dx*dx + dy*dy + dz*dz) < rmax in float64, d = x_j - x_i
  bin      k = (int)(r * inv_dr), inv_dr = nbins / rmax; counted when k < nbins
  centres  centres[p] = owned atoms of species a_p (per frame)

A harness.System is a whole box: every atom is a centre, the neighbours are all atoms and all their periodic images (enough shifts
per dimension to cover rmax even when L < rmax, an atom's own images included).  A harness.RankInput is one rank's share: its owned
atoms are the centres, the neighbours are its owned atoms plus its ghosts, as given (the ghost shell reaches beyond rmax).
"""
import itertools

import numpy as np

CHUNK = 64


def _atoms(obj):
    """(positions of the centres, their species, positions of all neighbours, their species); neighbour c is centre c itself"""
    if hasattr(obj, "nlocal"):
        x = np.asarray(obj.x, dtype=np.float64)
        sp = np.asarray(obj.species, dtype=np.int64)
        return x[: obj.nlocal], sp[: obj.nlocal], x, sp
    x = np.asarray(obj.x, dtype=np.float64)
    sp = np.asarray(obj.types, dtype=np.int64) - 1
    return x, sp, x, sp


def _shifts(obj, rmax):
    """image shifts in Angstrom, the zero shift first; a RankInput brings its images along as ghosts"""
    if hasattr(obj, "nlocal"):
        return np.zeros((1, 3))
    L = np.asarray(obj.boxhi, dtype=np.float64) - np.asarray(obj.boxlo, dtype=np.float64)
    reach = [int(np.ceil(rmax / L[k])) if obj.periodic[k] else 0 for k in range(3)]
    cells = [c for c in itertools.product(*[range(-m, m + 1) for m in reach]) if c != (0, 0, 0)]
    return np.array([(0, 0, 0)] + cells, dtype=np.float64) * L


def scan(obj, pairs, nbins, rmax):
    """(counts, centres, edge gap) in one pass: see counts() and edge_gap()"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    xc, sc, xa, sa = _atoms(obj)
    S = int(max(sa.max(initial=0), pairs.max(initial=0))) + 1
    slot_of = np.full((S, S), -1, dtype=np.int64)
    for p, (a, b) in enumerate(pairs.tolist()):
        assert slot_of[a, b] < 0, "duplicate pair"
        slot_of[a, b] = p
    inv_dr = nbins / rmax
    hist = np.zeros((len(pairs), nbins), dtype=np.uint64)
    gap = np.inf
    for sh_no, sh in enumerate(_shifts(obj, rmax)):
        xs = xa + sh
        for c0 in range(0, len(xc), CHUNK):
            c = np.arange(c0, min(c0 + CHUNK, len(xc)))
            d = xs[None, :, :] - xc[c][:, None, :]
            dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
            r = np.sqrt(dx * dx + dy * dy + dz * dz)
            if sh_no == 0:
                r[np.arange(len(c)), c] = np.inf       # the atom itself; its images are neighbours
            slot = slot_of[sc[c][:, None], sa[None, :]]
            near = (slot >= 0) & (r < rmax + 0.5 / inv_dr)
            t = r[near] * inv_dr
            if t.size:
                gap = min(gap, float(np.abs(t - np.rint(t)).min() / inv_dr))
            ok = (slot >= 0) & (r < rmax)
            k = (r[ok] * inv_dr).astype(np.int64)
            s = slot[ok]
            keep = k < nbins
            np.add.at(hist, (s[keep], k[keep]), 1)
    centres = np.array([(sc == a).sum() for a in pairs[:, 0]], dtype=np.uint64)
    return hist, centres, gap


class Case:
    """an input with its configuration and the reference's answer (computed once, never changed)"""

    def __init__(self, obj, pairs, nbins, rmax):
        self.obj, self.pairs, self.nbins, self.rmax = obj, np.asarray(pairs, dtype=np.int64).reshape(-1, 2), int(nbins), float(rmax)
        self.counts, self.centres, self.gap = scan(obj, self.pairs, self.nbins, self.rmax)
        for a in (self.pairs, self.counts, self.centres):
            a.setflags(write=False)

    @property
    def totals(self):
        return self.counts.sum(1).tolist()


ALL16 = [(a, b) for a in range(4) for b in range(4)]
SUBSET = [(0, 3), (0, 1), (2, 2)]   # species 0 is the centre of two histograms
RCR = 5.1                           # ANI-2x radial cutoff
_cases = {}


def random_system():
    from lammps_ani_amd import harness as hx
    return hx.random_box(600, 4, 16.0, seed=7)


def one_atom_system():
    from lammps_ani_amd import harness as hx
    return hx.System(np.array([[1.0, 1.5, 2.25]]), np.array([4], dtype=np.int32), np.zeros(3), np.full(3, 4.0))


def case(name):
    """the inputs the GPU tests use (tests/test_rdf.py); tests/test_rdf_reference_cpu.py pins their gaps and totals"""
    from lammps_ani_amd import harness as hx
    if name in _cases:
        return _cases[name]
    if name == "random":             # one rank, 3404 ghosts
        c = Case(hx.decompose(random_system()), ALL16, 64, RCR)
    elif name == "random_whole":     # the same box without a decomposition: images by shifts
        c = Case(random_system(), ALL16, 64, RCR)
    elif name == "random_4096":      # 65536 bins: the global-atomics path
        c = Case(case("random").obj, ALL16, 4096, RCR)
    elif name == "random_subset":
        c = Case(case("random").obj, SUBSET, 64, 2.0)
    elif name in ("rank0", "rank1"):
        c = Case(hx.decompose(random_system(), grid=(2, 1, 1), rank=int(name[-1])), ALL16, 64, RCR)
    elif name == "one_atom":         # L = 4 A < rmax: its own images are its only neighbours
        c = Case(hx.decompose(one_atom_system()), [(3, 3)], 64, RCR)
    else:
        raise KeyError(name)
    _cases[name] = c
    return c


def counts(sysm_or_inp, pairs, nbins, rmax):
    """(counts uint64 [npair, nbins], centres uint64 [npair]) of one frame; pairs: [npair, 2] species indices"""
    h, c, _ = scan(sysm_or_inp, pairs, nbins, rmax)
    return h, c


def edge_gap(sysm_or_inp, pairs, nbins, rmax):
    """smallest distance (Angstrom) of any counted or nearly counted pair (r below rmax plus half a bin) from a bin edge, 0 and rmax
    included: how far the input is from a pair whose bin the last bits of the arithmetic could move"""
    return scan(sysm_or_inp, pairs, nbins, rmax)[2]
