"""CPU reference of the molecule finder (ani_find_molecules, include/ani_hip.h), written from the definitions there and not from the
library: plain numpy / Python union-find over a harness.RankInput.

  bond      list entry (centre i, neighbour j) with |x_j - x_i|^2 <= cut[s_i][s_j]^2 in float64; an entry <= 0 never bonds
  owner     ghost g >= nlocal stands for owned atom owner[g - nlocal]; a value outside [0, nlocal) is a foreign ghost
  molecule  connected component of the owned atoms, ghosts replaced by their owners; label = smallest owned index
  open      a molecule with a bond to a foreign ghost: counted, labelled, left out of the formula table
  summary   molecules, distinct closed compositions, open molecules, directed bonds, largest molecule, owned atoms in open ones
"""
import json
import os

import numpy as np

SYMBOLS_ANI2X = ("H", "C", "N", "O", "S", "F", "Cl")


def load_table(symbols=SYMBOLS_ANI2X, path=None):
    """[S][S] bond table in Angstrom of tests/golden/bond_table_analysis.json (pairs it does not list: 0 = never bonded)"""
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bond_table_analysis.json")
    with open(path) as f:
        d = json.load(f)
    sym = list(symbols)
    t = np.zeros((len(sym), len(sym)))
    for pair, v in d["bond_lengths"].items():
        a = next(s for s in sorted(sym, key=len, reverse=True) if pair.startswith(s))
        b = pair[len(a):]
        if a in sym and b in sym:
            t[sym.index(a), sym.index(b)] = t[sym.index(b), sym.index(a)] = v + d["stretch_margin"]
    return t


def owners_of(inp, rank=0):
    """int64 [nghost]: the owned atom a ghost stands for, -1 for the ghosts of other ranks"""
    return np.where(np.asarray(inp.owner_rank) == rank, np.asarray(inp.owner_lidx), -1).astype(np.int64)


def candidate_pairs(inp, table, x=None):
    """(i, j, r, cut) of every list entry whose species pair can bond at all"""
    x = np.asarray(inp.x if x is None else x, dtype=np.float64)
    sp = np.asarray(inp.species)
    i = np.repeat(np.asarray(inp.ilist, dtype=np.int64), np.asarray(inp.numneigh))
    j = np.asarray(inp.jlist, dtype=np.int64)
    cut = np.asarray(table, dtype=np.float64)[sp[i], sp[j]]
    keep = cut > 0
    i, j, cut = i[keep], j[keep], cut[keep]
    d = x[j] - x[i]
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return i, j, r2, cut


def threshold_gap(inp, table, x=None):
    """smallest | r - cut | over the candidate pairs (Angstrom): how far the input is from a pair the arithmetic could flip"""
    _, _, r2, cut = candidate_pairs(inp, table, x)
    return float(np.abs(np.sqrt(r2) - cut).min()) if len(r2) else np.inf


def find_molecules(inp, table, owner=None, x=None):
    """owner: int64 [nghost] or None (every ghost foreign).  Returns (labels int32 [nlocal], {composition tuple: closed
    molecules}, summary int64 [6], image bonds: accepted entries whose neighbour is a ghost)."""
    nl = inp.nlocal
    S = np.asarray(table).shape[0]
    i, j, r2, cut = candidate_pairs(inp, table, x)
    bond = r2 <= cut * cut
    i, j = i[bond], j[bond]
    parent = list(range(nl))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    open_atom = np.zeros(nl, dtype=bool)
    for a, b in zip(i.tolist(), j.tolist()):
        o = b
        if b >= nl:
            o = int(owner[b - nl]) if owner is not None else -1
        if o < 0 or o >= nl:
            open_atom[a] = True
            continue
        ra, rb = find(a), find(o)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    labels = np.array([find(a) for a in range(nl)], dtype=np.int32)
    sp = np.asarray(inp.species)[:nl]
    formulas, n_open, open_atoms, largest = {}, 0, 0, 0
    roots = np.unique(labels)
    for r in roots.tolist():
        members = np.nonzero(labels == r)[0]
        assert members.min() == r
        largest = max(largest, len(members))
        if open_atom[members].any():
            n_open += 1
            open_atoms += len(members)
            continue
        comp = tuple(np.bincount(sp[members], minlength=S).tolist())
        formulas[comp] = formulas.get(comp, 0) + 1
    summary = np.array([len(roots), len(formulas), n_open, len(i), largest, open_atoms], dtype=np.int64)
    return labels, formulas, summary, int((j >= nl).sum())


def formula_rows(formulas):
    """the formula table as the host entry returns it: rows [n][S + 1], ascending lexicographically by composition"""
    return np.array([list(c) + [n] for c, n in sorted(formulas.items())], dtype=np.int32).reshape(len(formulas), -1)
