"""Helpers for the neighbour-list contract tests (tests/test_list_forms_cpu.py, tests/test_list_contract.py).  No GPU.

include/ani_hip.h lets a caller hand over the centres in any order: ``ilist_unique[nlocal]`` is an arbitrary ordering of the
owned atoms, ``numneigh[ii]`` and the jlist segments follow that order, ``out_atomic_energies`` / ``atom_energy_dev`` come back in
ilist order, and everything indexed by atom (forces, per-atom virial, member_dforce, atom_force_dev) does not care.  The functions
here rewrite a ``harness.RankInput`` into another FORM of the same list -- the same centres with the same neighbour sets, so the
same physics -- and say what a result of the identity form looks like in the other form.

The second half builds the inputs the two test modules share (``build_input``), each the smallest system that reaches one edge of
the rebuild-time code: the chunk boundaries of the preparation kernels and of the neighbour-count scan (4096 centres), rows of
length zero between dense ones, a species that only ghosts have.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from lammps_ani_amd import harness as hx

FORMS = ("reversed", "random", "random+shuffled")
FORM_SEED = 20240611

# keys of a result dict (Oracle.compute / ANI.compute) by what indexes them
BY_CENTRE = ("eatom", "aev", "gaev")
BY_CENTRE_DEVIATION = ("atom_energy_dev",)


def _offsets(numneigh):
    off = np.zeros(len(numneigh) + 1, dtype=np.int64)
    np.cumsum(numneigh, out=off[1:])
    return off


def segments(inp):
    """the jlist segments of ``inp`` as a list of arrays, in ilist order"""
    off = _offsets(inp.numneigh)
    return [inp.jlist[off[k]: off[k + 1]] for k in range(inp.nlocal)]


def reorder_centres(inp, perm):
    """centre ``perm[k]`` of ``inp`` becomes centre k: ilist and numneigh are gathered through perm, the segments are concatenated in
    perm order; the order INSIDE every segment is kept.  Full lists only."""
    assert not inp.half
    perm = np.asarray(perm, dtype=np.int64)
    assert np.array_equal(np.sort(perm), np.arange(inp.nlocal))
    off = _offsets(inp.numneigh)
    nn = inp.numneigh[perm].astype(np.int32)
    # entry e of the new jlist: position off[perm[k]] + (e - newoff[k]) of the old one, k the new centre of e
    newoff = _offsets(nn)
    src = np.repeat(off[perm] - newoff[:-1], nn) + np.arange(int(newoff[-1]), dtype=np.int64)
    jl = inp.jlist[src].astype(np.int32) if len(src) else np.zeros(0, np.int32)
    return dataclasses.replace(inp, ilist=inp.ilist[perm].astype(np.int32), numneigh=nn, jlist=jl)


def shuffle_segments(inp, rng):
    """every segment in a random order of its own (the centres stay where they are)"""
    assert not inp.half
    off = _offsets(inp.numneigh)
    jl = inp.jlist.copy()
    for k in range(inp.nlocal):
        a, b = off[k], off[k + 1]
        if b - a > 1:
            jl[a:b] = rng.permutation(jl[a:b])
    return dataclasses.replace(inp, jlist=jl)


def form_perm(form, nlocal, seed=FORM_SEED):
    if form == "identity":
        return np.arange(nlocal)
    if form == "reversed":
        return np.arange(nlocal)[::-1].copy()
    if form in ("random", "random+shuffled"):
        return np.random.default_rng(seed).permutation(nlocal)
    raise ValueError(form)


def apply_form(inp, form, seed=FORM_SEED):
    """(the input in that form, perm)"""
    perm = form_perm(form, inp.nlocal, seed)
    out = reorder_centres(inp, perm)
    if form == "random+shuffled":
        out = shuffle_segments(out, np.random.default_rng(seed + 1))
    return out, perm


def expected(ref, perm):
    """A result dict of the identity input as the reordered input must return it: what is indexed by centre (eatom,
    deviation["atom_energy_dev"], the oracle's aev / gaev rows) is gathered through perm; energy, force, virial, atom_virial,
    member_energy, member_dforce, atom_force_dev and summary are sums or indexed by atom and do not change.  (include/ani_hip.h:
    "per-centre energies in ilist order", atom_energy_dev "indexed like eatom", atom virial "indexed by atom (not in ilist
    order)".)"""
    perm = np.asarray(perm, dtype=np.int64)
    out = {}
    for k, v in ref.items():
        if k == "deviation" and v is not None:
            out[k] = {kk: (vv[perm] if kk in BY_CENTRE_DEVIATION else vv) for kk, vv in v.items()}
        elif k in BY_CENTRE and v is not None:
            out[k] = v[perm]
        else:
            out[k] = v
    return out


def longest_fixed_run(perm):
    """the longest run of consecutive k with perm[k] == k"""
    best = cur = 0
    for hit in (np.asarray(perm) == np.arange(len(perm))).tolist():
        cur = cur + 1 if hit else 0
        best = max(best, cur)
    return best


# ------------------------------------------------------------------------------------------------------------------
# the shared inputs
# ------------------------------------------------------------------------------------------------------------------

# id -> (model kind, members); the model seed is MODEL_SEED everywhere
MODEL_SEED = 2024
INPUT_MODELS = {
    "chunk4096": ("ani1x", 1), "chunk4097": ("ani1x", 1), "chunk8193": ("ani1x", 1),
    "cluster_isolated": ("ani1x", 2), "ghost_only_species": ("ani1x", 2), "mixed7_brick": ("ani2x", 2), "tiny_generic": ("tiny", 2),
}
INPUT_IDS = tuple(INPUT_MODELS)
CHUNK_NLOCAL = {"chunk4096": 4096, "chunk4097": 4097, "chunk8193": 8193}
N_ISOLATED = 5
GHOST_ONLY_TYPE = 3   # LAMMPS type of the species that only ghosts carry (species 2, N of H C N O)


def chunk_box(n):
    """4-species random box of n atoms at about 0.1 atoms / A^3 (34.5 A at 4097, 43.4 A at 8193)"""
    return hx.random_box(n, 4, round((n / 0.1) ** (1.0 / 3.0), 1), seed=n)


def cluster_system():
    """open boundaries: a dense 500-atom cluster and N_ISOLATED atoms 60 A out on the axes (84 A from each other), three of them in
    the middle of the atom order and two at its end"""
    s = hx.random_box(500, 4, 18.0)
    far = 60.0 * np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0]])
    far_types = np.array([1, 2, 3, 4, 1], dtype=np.int32)
    x = np.concatenate([s.x[:100], far[0:1], s.x[100:250], far[1:3], s.x[250:], far[3:5]])
    t = np.concatenate([s.types[:100], far_types[0:1], s.types[100:250], far_types[1:3], s.types[250:], far_types[3:5]])
    isolated = np.array([100, 251, 252, 503, 504])
    assert np.array_equal(x[isolated], far)
    return hx.System(x, t.astype(np.int32), np.full(3, -80.0), np.full(3, 80.0), (False, False, False)), isolated


def ghost_only_system():
    """random box whose lower half in x (rank 0's brick of a (2,1,1) grid) holds no atom of type GHOST_ONLY_TYPE: they are retyped
    to 2 there, the upper half keeps its own"""
    s = hx.random_box(1200, 4, 26.0, seed=21)
    t = s.types.copy()
    t[(t == GHOST_ONLY_TYPE) & (s.x[:, 0] < 0.0)] = 2
    return hx.System(s.x, t, s.boxlo, s.boxhi)


@functools.lru_cache(maxsize=None)
def build_input(name):
    """the identity-form RankInput of input ``name`` (cached: treat it as read-only, the forms copy)"""
    if name in CHUNK_NLOCAL:
        return hx.decompose(chunk_box(CHUNK_NLOCAL[name]))
    if name == "cluster_isolated":
        return hx.decompose(cluster_system()[0])
    if name == "ghost_only_species":
        return hx.decompose(ghost_only_system(), (2, 1, 1), 0)
    if name == "mixed7_brick":
        return hx.decompose(hx.random_box(2500, 7, 31.0, seed=4), (2, 2, 2), 5)
    if name == "tiny_generic":
        return hx.decompose(hx.random_box(300, 3, 16.0))
    raise KeyError(name)


def model_path(name, model_cache):
    kind, members = INPUT_MODELS[name]
    return model_cache(kind, members, MODEL_SEED)


def neighbours_within(inp, rc):
    """per centre (ilist order): how many entries of its segment lie inside rc"""
    i = np.repeat(inp.ilist.astype(np.int64), inp.numneigh)
    d = inp.x[inp.jlist] - inp.x[i]
    inside = (np.einsum("ij,ij->i", d, d) < rc * rc).astype(np.int64)
    off = _offsets(inp.numneigh)
    csum = np.concatenate([[0], np.cumsum(inside)])
    return csum[off[1:]] - csum[off[:-1]]
