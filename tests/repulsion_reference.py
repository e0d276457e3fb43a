"""Plain numpy fp64 reference of the pairwise repulsion (model-file block REPULXTB) ALONE, with derived bars and mutations.

No GPU and no oracle in here: tests/test_repulsion_reference_cpu.py checks this module against the oracle on null models, and
tests/test_repulsion_kernels.py checks the three kernel paths (folded into ``aev_backward_fast``, ``repulsion_kernel<float>``,
``repulsion_kernel<double>``) against it.

Formula (header of lammps-ani_amd/csrc/ani_kernels_rep.hip; oracle/ani_oracle.c:rep_pair), r in Angstrom, db = r * a2b in Bohr:

    g(r)  = y_ab / db * exp(-al_ab * db^k_ab)            dg = a2b * g * L,   L = -1/db - al k db^(k-1)
    fc(r) = exp(A1), A1 = 1 - 1/den, den = 1 - (r/Rc)^2  dfc = fc * P,       P = -(2 r / Rc^2) / den^2
    e(r)  = g fc,   e'(r) = dg fc + g dfc;   an entry is skipped when r >= Rc or den <= 1e-10.

Every (centre i, neighbour j) entry of the full list carries HALF of the pair: energy e/2, gradient dE/dx_j = (e'/2) d / r with
d = x_j - x_i.  A pair of two owned atoms is met from both ends, an owned-ghost pair from one end: a rank's share.

A *null network* (``null_model``) has every weight, bias and self energy zero, so that the outputs of a model file are the
repulsion alone: the network's row energies are exactly 0, its dE/dAEV exactly 0, and every AEV gradient is multiplied by it.

Bars.  The code under test never enters its own bar: bar = min(MARGIN * model, cap), model = the first-order error model below,
evaluated on the fp64 reference's own terms.

fp32 paths (u = 2^-24).  Both fp32 kernels take r from the fp64 positions, round it to float and evaluate the pair function in
fp32; for the half gradient s = e'/2 of one entry the model is

    |ds/dr| r u                                                     the rounding of r (e'' analytic, checked by differences)
  + u/2 * (|dg fc| (N + cA1 + cA2 + cL) + |g dfc| (N + cA1 + cA2 + cD))
        N   = 32   fp32 roundings on the way from r to a force component (7 for fc, 4 more for dfc, 10 for g, 6 for dg, 3 for
                   the sum, 2 for the component), each relative to its own term; no term is a difference of others except
                   den and A1, whose conditioning is counted apart:
        cA1 = (3 x^2 + den) / den^2 + 1/den + 3 |A1|   absolute error of the exponent A1 = relative error of fc: x^2 carries
                   three roundings, den = 1 - x^2 one more, the reciprocal one, the subtraction and the scaling by log2(e) three
        cA2 = |A2| (cP + 4), A2 = al db^k      the exponent of g: db^(k-1) = exp2((k-1) log2 db) is good to cP = 3 ln2 |B| + 1
                   roundings, B = (k-1) log2 db (three roundings of the exponent B, one of exp2), four more for the products
        cL  = cP + 3                           L = -1/db - al k db^(k-1), both terms of one sign
        cD  = 2 (3 x^2 / den + 1) + 3          the 1/den^2 of P
  then per atom: the sum over the entries whose gradient lands on it (as centre and as neighbour), plus the fp32 accumulation
  into fbuf: at most n + 1 float additions (atomics in any order) of partial sums no larger than scale = sum |s|:
  (n + 1) u scale.
  Energy: |e'/2| r u + |e/2| (N_E + cA1 + cA2) u per entry, N_E = 20; the folded path sums a wave's entries in a float (at these
  sizes a wave of the persistent grid takes one centre: ceil(longest list / 64) additions per lane and six for the wave sum)
  before the double slots: (ceil(nmax / 64) + 6) u sum |e/2|.
  Virial and atom virial: |d| times the entry's gradient error, plus |s| times the error of the displacement (the folded path
  takes d from the fp32 packed positions: three roundings of a coordinate, 3 u max|x|, and two for the product), plus the float
  accumulation as above (per centre for the virial, per atom for the atom virial).
  Underflow: fp32 products below 2^-126 and denormal results of the hardware exp2 are flushed to zero, and factors of up to
  2^26 (1/den^2 next to the cutoff) multiply such a value: every live entry carries an absolute 2^-100 (atomic units) on top.
  MARGIN = 8 over this model for the hardware exp2 / log2 / rcp (1 to 2 ulp against the 0.5 assumed), as tests/aev_edges.py
  justifies it.  Caps: forces max(F_TOL, 2e-5 max|F_ref|) (tests/test_baseline_workloads.py), energy E_TOL_PER_ATOM nlocal,
  virial V_TOL max(1, nlocal / 100), atom virial Rcr * force cap * n_j (tests/test_atom_virial.py with the force cap above).

fp64 paths (u = 2^-53): the same model with N = 64 (the 32 operations, exp at 3 ulp twice and pow at 16 ulp twice, the bounds of
the OpenCL profile the device's libm follows) and cP = 16 (pow), times 2 because this reference is an fp64 evaluation of the same
conditioning; r = sqrt(d.d) carries 3 roundings instead of one.  Caps: the existing fp64 bars, F 1e-8, E 9e-9 |E|, V 1e-6.
"""
import dataclasses

import numpy as np

from lammps_ani_amd import harness as hx
from lammps_ani_amd import model_file as mf

KCAL = 627.5094738898777
A2B = 1.8897261258369282
U32, U64 = 2.0 ** -24, 2.0 ** -53
MARGIN = 8.0
TINY = 2.0 ** -100                 # see "underflow" in the module docstring
F_TOL, F_REL = 2.3e-3, 2e-5        # tests/test_baseline_workloads.py
E_TOL_PER_ATOM = 1e-5
V_TOL = 2e-2
F_TOL64, E_REL64, V_TOL64 = 1e-8, 9e-9, 1e-6
CVATOM = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2), (1, 0), (2, 0), (2, 1)]
MODEL_SEED = 2024


def null_model(m, repulsion="keep"):
    """``m`` with every weight, bias and self energy zero; repulsion: the block to carry (default: m's own), None = no block"""
    w = [[[(np.zeros_like(W), np.zeros_like(b)) for W, b in per_l] for per_l in per_s] for per_s in m.weights]
    return dataclasses.replace(m, self_energies=np.zeros(len(m.species)), weights=w,
                               repulsion=m.repulsion if isinstance(repulsion, str) else repulsion)


def _pair_function(r, y, al, k, cut, real, no_dfc=False):
    """e/2 and e'/2 (Hartree, Hartree/A) of the entries; real = float32: the arithmetic of the fp32 kernels, operation by operation"""
    if real is np.float32:
        f = np.float32
        rf, rc = r.astype(f), f(cut)
        x = rf / rc
        den = f(1) - x * x
        ok = (r < cut) & (den > f(1e-10))
        den = np.where(ok, den, f(1))
        l2e = f(1.4426950408889634)
        fc = np.exp2((f(1) - f(1) / den) * l2e)
        dfc = fc * (-(f(2) * x / rc) / (den * den))
        db = np.where(ok, rf, f(1)) * f(A2B)
        alf, kf = al.astype(f), k.astype(f)
        pk1 = np.exp2((kf - f(1)) * np.log2(db))
        g = y.astype(f) / db * np.exp2(-alf * pk1 * db * l2e)
        dg = f(A2B) * g * (f(-1) / db - alf * kf * pk1)
        if no_dfc:
            dfc = np.zeros_like(dfc)
        eh = f(0.5) * (g * fc)
        sh = f(0.5) * (dg * fc + g * dfc)
        return ok, np.where(ok, eh, 0).astype(np.float64), np.where(ok, sh, 0).astype(np.float64)
    x = r / cut
    den = 1.0 - x * x
    ok = (r < cut) & (den > 1e-10)
    den = np.where(ok, den, 1.0)
    fc = np.exp(1.0 - 1.0 / den)
    dfc = fc * (-(2.0 * x / cut) / (den * den))
    db = np.where(ok, r, 1.0) * A2B
    g = y / db * np.exp(-al * db ** k)
    dg = A2B * g * (-1.0 / db - al * k * db ** (k - 1.0))
    if no_dfc:
        dfc = np.zeros_like(dfc)
    return ok, np.where(ok, 0.5 * g * fc, 0.0), np.where(ok, 0.5 * (dg * fc + g * dfc), 0.0)


def pair_terms(inp, rep, real=np.float64, mutation=None, Rcr=None):
    """Per full-list entry: i, j, d = x_j - x_i (fp64 positions), r, the half pair energy eh (Hartree), the half pair gradient
    g = dE/dx_j (Hartree/A), and the table entries y, al, k it used.  mutation: a key of MUTATIONS (Rcr for "beyond_rcr")."""
    i = np.repeat(np.asarray(inp.ilist, dtype=np.int64), inp.numneigh)
    j = np.asarray(inp.jlist, dtype=np.int64)
    d = inp.x[j] - inp.x[i]
    r = np.sqrt((d * d).sum(1))
    sp = np.asarray(inp.species, dtype=np.int64)
    if mutation == "compact_tables":   # tables read at the index among the species present
        present = np.unique(sp)
        sp = np.searchsorted(present, sp)
    sa, sb = sp[i], sp[j]
    kt = rep["k_rep_ab"]
    if mutation == "k_hh":
        kt = kt.copy()
        kt[0, 0] = 1.5
    y, al, k = rep["y_ab"][sa, sb], rep["sqrt_alpha_ab"][sa, sb], kt[sa, sb]
    ok, eh, sh = _pair_function(r, y, al, k, float(rep["cutoff"]), real, no_dfc=(mutation == "no_dfc"))
    if mutation == "beyond_rcr":
        keep = r <= Rcr
        eh, sh = np.where(keep, eh, 0.0), np.where(keep, sh, 0.0)
    if mutation == "ghost_whole":
        w = np.where(j >= inp.nlocal, 2.0, 1.0)
        eh, sh = eh * w, sh * w
    if mutation == "energy_whole":
        eh = 2.0 * eh
    g = (sh / np.where(r > 0, r, 1.0))[:, None] * d
    return dict(i=i, j=j, d=d, r=r, eh=eh, sh=sh, g=g, y=y, al=al, k=k, cut=float(rep["cutoff"]))


def rep_terms(inp, rep):
    """half-pair repulsion of every full-list entry (i, j): d = x_j - x_i, g = dE/dx_j (Hartree/A); oracle/ani_oracle.c:rep_pair"""
    t = pair_terms(inp, rep)
    return t["i"], t["j"], t["d"], t["g"]


def to_ncomp(W, ncomp):
    """[n, 3, 3] -> [n, ncomp] in LAMMPS order (atom_virial_kernel: 9 = xx yy zz xy xz yz yx zx zy, 6 = the symmetric part)"""
    if ncomp == 9:
        return np.stack([W[:, a, b] for a, b in CVATOM], axis=1)
    S = 0.5 * (W + W.transpose(0, 2, 1))
    return np.stack([S[:, a, b] for a, b in CVATOM[:6]], axis=1)


def reference(inp, rep, real=np.float64, mutation=None, Rcr=None):
    """force [ntotal, 3] (kcal/mol/A), energy (kcal/mol, the rank's share: half per entry), virial [3, 3] (sign and symmetrisation
    of the oracle's pass C), atom_virial(ncomp) -> [ntotal, ncomp] (W_j = sum d (x) F_j over the entries landing on j, the order
    and sign of atom_virial_kernel), scale [ntotal] = sum over an atom's terms of |g| (kcal/mol/A), nterms [ntotal], terms."""
    t = pair_terms(inp, rep, real, mutation, Rcr)
    nt = inp.ntotal
    i, j, d, g = t["i"], t["j"], t["d"], t["g"]
    F = np.zeros((nt, 3))
    np.add.at(F, j, -KCAL * g)
    np.add.at(F, i, KCAL * g)
    V = -KCAL * np.einsum("pk,pl->kl", g, d)
    W = np.zeros((nt, 3, 3))
    np.add.at(W, j, -KCAL * d[:, :, None] * g[:, None, :])
    mag = KCAL * np.abs(t["sh"])
    scale = np.zeros(nt)
    np.add.at(scale, j, mag)
    np.add.at(scale, i, mag)
    nterms = np.zeros(nt, dtype=np.int64)
    nz = (t["sh"] != 0).astype(np.int64)
    np.add.at(nterms, j, nz)
    np.add.at(nterms, i, nz)
    return dict(force=F, energy=KCAL * float(t["eh"].sum()), virial=0.5 * (V + V.T), W=W, atom_virial=lambda ncomp: to_ncomp(W, ncomp),
                scale=scale, nterms=nterms, terms=t)


def second_derivative(t):
    """e''(r)/2 of every entry (Hartree/A^2), analytic: e'' = g fc ((L^2 + L') + 2 L P + (P^2 + P'))"""
    r, al, k, cut = t["r"], t["al"], t["k"], t["cut"]
    live = t["sh"] != 0
    rr = np.where(live, r, 1.0)
    den = np.where(live, 1.0 - (rr / cut) ** 2, 1.0)
    db = rr * A2B
    L = A2B * (-1.0 / db - al * k * db ** (k - 1.0))
    Lp = A2B * A2B * (1.0 / db ** 2 - al * k * (k - 1.0) * db ** (k - 2.0))
    P = -(2.0 * rr / cut ** 2) / den ** 2
    Pp = -(2.0 / cut ** 2) / den ** 2 - (8.0 * rr * rr / cut ** 4) / den ** 3
    return np.where(live, t["eh"] * ((L * L + Lp) + 2.0 * L * P + (P * P + Pp)), 0.0)


def entry_errors(t, fp64=False):
    """first-order error bounds per entry (module docstring): of the half gradient s (Hartree/A) and of the half energy (Hartree)"""
    u = U64 if fp64 else U32
    r, al, k, cut = t["r"], t["al"], t["k"], t["cut"]
    live = t["sh"] != 0
    rr = np.where(live, r, 1.0)
    x2 = (rr / cut) ** 2
    den = np.where(live, 1.0 - x2, 1.0)
    db = rr * A2B
    A1 = 1.0 - 1.0 / den
    A2 = al * db ** k
    B = (k - 1.0) * np.log2(db)
    cP = np.full_like(rr, 16.0) if fp64 else 3.0 * np.log(2.0) * np.abs(B) + 1.0
    cA1 = (3.0 * x2 + den) / den ** 2 + 1.0 / den + 3.0 * np.abs(A1)
    cA2 = np.abs(A2) * (cP + 4.0)
    cL = cP + 3.0
    cD = 2.0 * (3.0 * x2 / den + 1.0) + 3.0
    N, NE = (64.0, 40.0) if fp64 else (32.0, 20.0)
    eh = t["eh"]                                            # g fc / 2
    Lr = A2B * (-1.0 / db - al * k * db ** (k - 1.0))       # dg = g L
    P = -(2.0 * rr / cut ** 2) / den ** 2                   # dfc = fc P
    t1, t2 = np.abs(eh * Lr), np.abs(eh * P)                # |dg fc| / 2, |g dfc| / 2
    nr = 3.0 if fp64 else 1.0
    es = np.abs(second_derivative(t)) * rr * u * nr + u * (t1 * (N + cA1 + cA2 + cL) + t2 * (N + cA1 + cA2 + cD))
    ee = np.abs(t["sh"]) * rr * u * nr + np.abs(eh) * (NE + cA1 + cA2) * u
    both = 2.0 if fp64 else 1.0                             # fp64: the reference is an evaluation of the same kind
    return np.where(live, es * both + TINY, 0.0), np.where(live, ee * both + TINY, 0.0)


def error_model(inp, ref, fp64=False):
    """the model, without margin and caps: force [ntotal], energy, virial, atom_virial [ntotal] (kcal/mol(/A))"""
    t = ref["terms"]
    u = U64 if fp64 else U32
    es, ee = entry_errors(t, fp64)
    i, j = t["i"], t["j"]
    nt = inp.ntotal
    f = np.zeros(nt)
    np.add.at(f, j, KCAL * es)
    np.add.at(f, i, KCAL * es)
    f += (ref["nterms"] + 1) * u * ref["scale"]
    nmax = int(np.max(inp.numneigh)) if len(inp.numneigh) else 0
    depth = (nmax + 63) // 64 + 6
    e = KCAL * float(ee.sum()) + depth * u * KCAL * float(np.abs(t["eh"]).sum())
    dl = np.sqrt((t["d"] ** 2).sum(1))
    xmax = float(np.abs(inp.x).max())
    sa = KCAL * np.abs(t["sh"])
    dd = 0.0 if fp64 else 3.0 * u * xmax                    # fp64: d from the fp64 positions, its rounding is in N
    per = dl * KCAL * es + sa * (dd + 2.0 * u * dl)
    v = float(per.sum()) + depth * u * float((dl * sa).sum())
    av = np.zeros(nt)
    np.add.at(av, j, per)
    avs = np.zeros(nt)
    np.add.at(avs, j, dl * sa)
    nj = np.zeros(nt)
    np.add.at(nj, j, (t["sh"] != 0).astype(np.float64))
    av += (nj + 1) * u * avs
    return dict(force=f, energy=e, virial=v, atom_virial=av, nj=nj)


def bars(inp, ref, Rcr, fp64=False):
    """bar = min(margin * model, cap) per output; returns dict(force [ntotal], energy, virial, atom_virial [ntotal], cap={...},
    model={...}).  fp64: margin 1 (the factor 2 for the reference is inside the model), caps the existing fp64 bars."""
    mdl = error_model(inp, ref, fp64)
    fmax = float(np.abs(ref["force"]).max())
    if fp64:
        cap = dict(force=F_TOL64, energy=E_REL64 * abs(ref["energy"]), virial=V_TOL64, atom_virial=Rcr * F_TOL64 * np.maximum(mdl["nj"], 1))
        margin = 1.0
    else:
        fcap = max(F_TOL, F_REL * fmax)
        cap = dict(force=fcap, energy=E_TOL_PER_ATOM * inp.nlocal, virial=V_TOL * max(1.0, inp.nlocal / 100.0),
                   atom_virial=Rcr * fcap * np.maximum(mdl["nj"], 1))
        margin = MARGIN
    out = {q: np.minimum(margin * mdl[q], cap[q]) for q in ("force", "energy", "virial", "atom_virial")}
    out["energy"], out["virial"] = float(out["energy"]), float(out["virial"])
    out.update(cap=cap, model=mdl, margin=margin)
    return out


def ratio(err, bar):
    """err / bar elementwise; where the bar is 0 (an atom no term lands on) 0 for an exact 0 and inf otherwise"""
    err, bar = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(bar, dtype=np.float64), np.shape(err))
    out = np.where(err == 0, 0.0, np.inf)
    np.divide(err, bar, out=out, where=bar > 0)
    return out


# ---- reference variants with one subtle fault each: name -> (what it is, applies(inp, rep, Rcr)) ------------------------------
MUTATIONS = {
    "beyond_rcr": ("the pairs with r > Rcr are dropped", lambda inp, rep, Rcr: rep["cutoff"] > Rcr),
    "compact_tables": ("tables indexed by compact species index instead of model species index",
                       lambda inp, rep, Rcr: len(np.unique(inp.species)) < rep["y_ab"].shape[0]),
    "k_hh": ("k_rep of H-H is 1.5", lambda inp, rep, Rcr: bool(np.any(inp.species == 0))),
    "no_dfc": ("the cutoff derivative dfc is omitted", lambda inp, rep, Rcr: True),
    "ghost_whole": ("the ghost entries count whole instead of half", lambda inp, rep, Rcr: inp.nghost > 0),
    "energy_whole": ("the half factor is dropped from the energy only", lambda inp, rep, Rcr: True),
}


def mutation_ratios(inp, rep, Rcr, ref, bar):
    """name -> the largest |mutated - reference| / bar over the atoms' force components and the energy, for the mutations that apply"""
    out = {}
    for name, (_, applies) in MUTATIONS.items():
        if not applies(inp, rep, Rcr):
            continue
        mut = reference(inp, rep, mutation=name, Rcr=Rcr)
        rf = float(ratio(np.abs(mut["force"] - ref["force"]).max(1), bar["force"]).max())
        re = abs(mut["energy"] - ref["energy"]) / bar["energy"]
        out[name] = max(rf, re)
    return out


# ---- the cases of tests/test_repulsion_kernels.py: id -> model kind, block, system, list ------------------------------------------
def _open_cluster(n, ntypes, seed):
    s = hx.random_box(n, ntypes, 7.0, seed=seed, min_dist=1.0)
    return hx.System(s.x, s.types, s.boxlo - 20.0, s.boxhi + 20.0, (False, False, False))


SEVEN = dict(n=216, L=10.6, seed=5, min_dist=1.45)   # chosen on the reference alone: max|F| < 2000, longest radial list > 64

CASES = {
    # id: (kind, block edit, system factory, decompose keywords beyond cutoff = Rcr)
    "mixed64": ("ani1x", {}, lambda: hx.random_box(64, 4, 9.0, seed=11), {}),
    "mixed64-cut51": ("ani1x", {"cutoff": 5.1}, lambda: hx.random_box(64, 4, 9.0, seed=11), {}),
    "water-HO": ("ani1x", {}, lambda: hx.water_box(96), {}),
    "seven": ("ani2x", {}, lambda: hx.random_box(SEVEN["n"], 7, SEVEN["L"], seed=SEVEN["seed"], min_dist=SEVEN["min_dist"]), {}),
    "tiny64": ("tiny", {}, lambda: hx.random_box(64, 3, 9.0, seed=11), {}),
    "open40-ani1x": ("ani1x", {}, lambda: _open_cluster(40, 4, 21), {}),
    "open40-tiny": ("tiny", {}, lambda: _open_cluster(40, 3, 21), {}),
    # sqrt_alpha x 0.2 makes the term long-ranged, and the energy cap is absolute: one rounding of relative size u = 2^-24 that
    # goes the same way in every term (a constant rounded to float) moves the energy by u |E|, so a case whose MARGIN u |E|
    # exceeds E_TOL_PER_ATOM nlocal tests the cap and not the kernel (the CPU module asserts this for every case).  In the 9 A
    # box of mixed64 |E| is 7.9e4 kcal/mol (ratio 59); this thin box has 375 kcal/mol (0.28), with 0.15 kcal/mol/A and
    # 0.12 kcal/mol from the 164 entries between Rcr and the block's cutoff
    "soft-cut60": ("ani1x", {"cutoff": 6.0, "alpha_scale": 0.2}, lambda: hx.random_box(64, 4, 20.0, seed=3, min_dist=2.8),
                   {"cutoff": 6.0, "skin": 0.3}),
}
_CACHE = {}


def case_model(case, repulsion=True):
    """the null model of a case (repulsion=False: without the block)"""
    kind, edit, _, _ = CASES[case]
    m = mf.synthetic_model(kind, 1, MODEL_SEED, repulsion=True)
    rep = dict(m.repulsion)
    if "cutoff" in edit:
        rep["cutoff"] = float(edit["cutoff"])
    if "alpha_scale" in edit:
        rep["sqrt_alpha_ab"] = rep["sqrt_alpha_ab"] * edit["alpha_scale"]
    return null_model(m, rep if repulsion else None)


def case_system(case):
    if ("sys", case) not in _CACHE:
        _CACHE[("sys", case)] = CASES[case][2]()
    return _CACHE[("sys", case)]


def case_input(case, grid=(1, 1, 1), rank=0):
    """the RankInput of a case (cached): decompose(cutoff = Rcr) with the default skin unless the case says otherwise"""
    key = ("inp", case, grid, rank)
    if key not in _CACHE:
        m = case_model(case)
        kw = dict(cutoff=m.Rcr)
        kw.update(CASES[case][3])
        _CACHE[key] = hx.decompose(case_system(case), grid, rank, **kw)
    return _CACHE[key]


def case_reference(case, grid=(1, 1, 1), rank=0):
    """(inp, model, reference, bars fp32, bars fp64) of a case, computed once and left unchanged"""
    key = ("ref", case, grid, rank)
    if key not in _CACHE:
        inp, m = case_input(case, grid, rank), case_model(case)
        ref = reference(inp, m.repulsion)
        _CACHE[key] = (inp, m, ref, bars(inp, ref, m.Rcr), bars(inp, ref, m.Rcr, fp64=True))
    return _CACHE[key]
