"""numpy forms of the umbrella restraints, written from the contract in include/ani_md.h (ani_md_restraints_eval /
ani_md_restraints_apply): the reference of every restraint test, in float64 and np.longdouble.

From the header.  A restraint names 2, 3 or 4 atoms (slots a, b, c, d), a kind, kappa >= 0 and a centre.  Every difference vector is
a minimum image, minimg(a)[k] = a[k] - len[k] rint(a[k] / len[k]) in the periodic dimensions.
  distance  r = minimg(x_a - x_b), cv = |r|;  dcv/dx_a = r / |r| = -dcv/dx_b
  angle     u = minimg(x_a - x_b), w = minimg(x_c - x_b), c = u^ . w^ clamped, cv = acos(c), s = sqrt((1 - c)(1 + c));
            dcv/dx_a = (c u^ - w^) / (|u| s), dcv/dx_c = (c w^ - u^) / (|w| s), dcv/dx_b = minus their sum
  torsion   F = minimg(x_a - x_b), G = minimg(x_b - x_c), H = minimg(x_d - x_c), A = F x G, B = H x G, cv = atan2(-|G| F . B, A . B);
            T = (F . G) / (|A|^2 |G|) A - (H . G) / (|B|^2 |G|) B;  dcv/dx_a = -|G| / |A|^2 A, dcv/dx_d = |G| / |B|^2 B,
            dcv/dx_b = -dcv/dx_a + T, dcv/dx_c = -dcv/dx_d - T
  bias      D = cv - centre (torsion: D -= 2 pi rint(D / 2 pi), then + 2 pi where D <= -pi);  e = kappa / 2 D^2;  F_i = -kappa D dcv/dx_i
  virial    W_ab = sum_i rho_i,a F_i,b, rho relative to slot b: (r, 0), (u, 0, w), (F, 0, -G, H - G)
  not finite (D or any gradient entry): e = NaN, zero forces and virial, counted.
  apply     per touched atom the slot forces summed in the order (restraint, slot) ascending from 0, then f[i] += that;  E and W summed
            over the restraints;  ev[0] += E, with_virial: ev[1..10) += W;  record [0] evaluations [1] E [2..11) W [11] non-finite
            [12] largest |D| among the finite ones [13] words of the gather table that point outside (skipped; any makes E NaN).

Bars of the device test (`evaluation_bars`), the recipe of npt_reference.half_step_bars: per output ten times the difference between
`evaluate` in float64 and in np.longdouble on that case, floored at 1e-14 of the sum of the magnitudes of the terms the output is made
of.  The magnitudes, by Euclidean norms of the vectors involved (a cross product's small component carries the rounding of its large
terms): cv: |cv| for a distance, |cv| + 1 for an angle or a torsion (the rounding of the ratio that acos / atan2 see is an absolute
error in radians);  D: that + |centre|;  e: kappa / 2 (magnitude of D)^2;  a slot force: kappa (magnitude of D) times the summed
norms of the gradient's terms;  w: sum_i |rho_i| times the slot force magnitude;  an atom's accumulated force, E and W: the sums of
those;  what is added into f or ev: plus the magnitude of what was there.
"""
import numpy as np

from nh_reference import FTM2V, MVV2E

DISTANCE, ANGLE, TORSION = 0, 1, 2
KIND = {"distance": DISTANCE, "angle": ANGLE, "torsion": TORSION}
NATOMS_OF = {DISTANCE: 2, ANGLE: 3, TORSION: 4}
NREC = 16
TWOPI, PI = 6.283185307179586, 3.141592653589793          # the doubles of the kernel, in every precision


def minimg(a, length, pmask=7):
    a = np.array(a)
    for k in range(3):
        if (pmask >> k) & 1:
            a[..., k] = a[..., k] - length[k] * np.rint(a[..., k] / length[k])
    return a


def fold_delta(cv, centre, kind, dtype=np.float64):
    f = dtype
    d = f(cv) - f(centre)
    if kind == TORSION:
        d = d - f(TWOPI) * np.rint(d / f(TWOPI))
        if d <= -f(PI):
            d = d + f(TWOPI)
    return d


def _norm(a):
    return np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def collective_variable(kind, p, length, pmask=7, dtype=np.float64):
    """(cv, g [4, 3], rho [4, 3], gmag [4]) of one restraint from its atoms' positions p [4, 3] (unused rows ignored); gmag: the summed
    norms of the terms of each slot's gradient."""
    f = dtype
    p = np.asarray(p, dtype=dtype)
    L = np.asarray(length, dtype=dtype)
    g, rho, gmag = np.zeros((4, 3), dtype=dtype), np.zeros((4, 3), dtype=dtype), np.zeros(4, dtype=dtype)
    with np.errstate(all="ignore"):
        if kind == DISTANCE:
            r = minimg(p[0] - p[1], L, pmask)
            cv = _norm(r)
            g[0], g[1], rho[0] = r / cv, -(r / cv), r
            gmag[0] = gmag[1] = _norm(g[0])
        elif kind == ANGLE:
            u, w = minimg(p[0] - p[1], L, pmask), minimg(p[2] - p[1], L, pmask)
            lu, lw = _norm(u), _norm(w)
            uh, wh = u / lu, w / lw
            c = np.minimum(f(1.0), np.maximum(f(-1.0), _dot(uh, wh)))
            cv = np.arccos(c)
            s = np.sqrt((f(1.0) - c) * (f(1.0) + c))
            g[0], g[2] = (c * uh - wh) / (lu * s), (c * wh - uh) / (lw * s)
            g[1] = -(g[0] + g[2])
            rho[0], rho[2] = u, w
            gmag[0], gmag[2] = (abs(c) + f(1.0)) / (lu * s), (abs(c) + f(1.0)) / (lw * s)
            gmag[1] = gmag[0] + gmag[2]
        elif kind == TORSION:
            F, G, H = minimg(p[0] - p[1], L, pmask), minimg(p[1] - p[2], L, pmask), minimg(p[3] - p[2], L, pmask)
            A, B = np.cross(F, G), np.cross(H, G)
            lg, A2, B2 = _norm(G), _dot(A, A), _dot(B, B)
            cv = np.arctan2(-(lg * _dot(F, B)), _dot(A, B))
            ca, cb, ta, tb = lg / A2, lg / B2, _dot(F, G) / (A2 * lg), _dot(H, G) / (B2 * lg)
            T = ta * A - tb * B
            g[0], g[3] = -(ca * A), cb * B
            g[1], g[2] = T - g[0], -g[3] - T
            rho[0], rho[2], rho[3] = F, -G, H - G
            tmag = abs(ta) * _norm(A) + abs(tb) * _norm(B)
            gmag[0], gmag[3] = _norm(g[0]), _norm(g[3])
            gmag[1], gmag[2] = gmag[0] + tmag, gmag[3] + tmag
        else:
            raise ValueError(f"unknown kind {kind}")
    return cv, g, rho, gmag


def evaluate(x, atoms, kind, kappa, centre, length, pmask=7, dtype=np.float64):
    """ani_md_restraints_eval and the sums of ani_md_restraints_apply on positions x [n, 3] with the tables atoms [nr, 4] (-1 unused),
    kind [nr], kappa [nr], centre [nr].  Returns a dict: cv, delta, e [nr], fslot [nr, 4, 3], w [nr, 9], facc [n, 3] (what apply adds
    to f), E, W [9], nonfinite, max_delta, and the magnitudes of the module docstring: cv_mag, e_mag [nr], fslot_mag [nr, 4], w_mag
    [nr, 9], facc_mag [n], E_mag, W_mag [9]."""
    f = dtype
    x = np.asarray(x, dtype=np.float64)
    atoms = np.asarray(atoms, dtype=np.int64).reshape(-1, 4)
    nr, n = atoms.shape[0], x.shape[0]
    out = dict(cv=np.zeros(nr, dtype), delta=np.zeros(nr, dtype), e=np.zeros(nr, dtype), fslot=np.zeros((nr, 4, 3), dtype),
               w=np.zeros((nr, 9), dtype), cv_mag=np.zeros(nr), e_mag=np.zeros(nr), fslot_mag=np.zeros((nr, 4)), w_mag=np.zeros((nr, 9)))
    nonfinite, max_delta = 0, f(0.0)
    for r in range(nr):
        kd, kap = int(kind[r]), f(kappa[r])
        na = NATOMS_OF[kd]
        p = np.zeros((4, 3), dtype=dtype)
        p[:na] = x[atoms[r, :na]].astype(dtype)
        cv, g, rho, gmag = collective_variable(kd, p, length, pmask, dtype)
        with np.errstate(all="ignore"):
            d = fold_delta(cv, centre[r], kd, dtype)
            out["cv"][r], out["delta"][r] = cv, d
            if not (np.isfinite(d) and np.isfinite(g).all()):
                out["e"][r] = np.nan
                nonfinite += 1
                continue
            fr = -((kap * d) * g)
            out["e"][r] = (f(0.5) * kap) * (d * d)
            out["fslot"][r] = fr
            out["w"][r] = (((rho[0][:, None] * fr[0][None, :] + rho[1][:, None] * fr[1][None, :]) + rho[2][:, None] * fr[2][None, :])
                           + rho[3][:, None] * fr[3][None, :]).reshape(9)
            max_delta = max(max_delta, abs(d))
            cvm = float(abs(cv)) + (0.0 if kd == DISTANCE else 1.0)
            dm = cvm + abs(float(centre[r]))
            out["cv_mag"][r] = cvm
            out["e_mag"][r] = 0.5 * float(kap) * dm * dm
            out["fslot_mag"][r] = float(kap) * dm * gmag.astype(np.float64)
            rn = np.sqrt((rho.astype(np.float64) ** 2).sum(1))
            out["w_mag"][r] = float((rn * out["fslot_mag"][r]).sum())
    facc, facc_mag = np.zeros((n, 3), dtype), np.zeros(n)
    for i in np.unique(atoms[atoms >= 0]):
        acc = np.zeros(3, dtype)
        for r, m in zip(*np.nonzero(atoms == i)):             # (restraint, slot) ascending
            acc = acc + out["fslot"][r, m]
            facc_mag[i] += out["fslot_mag"][r, m]
        facc[i] = acc
    E, W = f(0.0), np.zeros(9, dtype)
    for r in range(nr):
        E = E + out["e"][r]
        W = W + out["w"][r]
    out.update(facc=facc, facc_mag=facc_mag, E=E, W=W, nonfinite=nonfinite, max_delta=max_delta, E_mag=float(out["e_mag"].sum()),
               W_mag=out["w_mag"].sum(0))
    return out


def evaluation_bars(x, atoms, kind, kappa, centre, length, pmask=7):
    """(reference in float64, bars): absolute bars per output of the two kernels, the recipe of the module docstring; keys cv, e,
    fslot, w, facc, E, W (the bars of f and ev add the magnitude of what was there: the caller's)."""
    a = evaluate(x, atoms, kind, kappa, centre, length, pmask, np.float64)
    b = evaluate(x, atoms, kind, kappa, centre, length, pmask, np.longdouble)
    diff = {k: 10.0 * np.abs(np.asarray(a[k], dtype=np.longdouble) - b[k]).astype(np.float64) for k in ("cv", "e", "fslot", "w", "facc", "E", "W")}
    diff = {k: np.nan_to_num(v, nan=0.0) for k, v in diff.items()}       # NaN energies agree as NaN
    floor = dict(cv=a["cv_mag"], e=a["e_mag"], fslot=a["fslot_mag"][:, :, None], w=a["w_mag"], facc=a["facc_mag"][:, None], E=a["E_mag"],
                 W=a["W_mag"])
    return a, {k: np.maximum(diff[k], 1e-14 * np.asarray(floor[k])) for k in diff}


def tables(restraints):
    """(atoms [nr, 4], kind, kappa, centre) from a list of (kind name, atom indices, kappa, centre)"""
    nr = len(restraints)
    atoms = np.full((nr, 4), -1, dtype=np.int32)
    kind, kappa, centre = np.zeros(nr, dtype=np.int32), np.zeros(nr), np.zeros(nr)
    for r, (name, idx, kap, cen) in enumerate(restraints):
        kind[r], kappa[r], centre[r] = KIND[name], kap, cen
        atoms[r, : len(idx)] = idx
    return atoms, kind, kappa, centre


def bias(x, restraints, length, pmask=7):
    """(forces [n, 3], energy, virial [3, 3], evaluation dict) of a list of restraints on positions x"""
    ev = evaluate(x, *tables(restraints), length, pmask)
    return ev["facc"], float(ev["E"]), ev["W"].reshape(3, 3), ev


def biased(evaluate_model, restraints, with_virial=True):
    """an evaluate(x, lo, len) -> (f, pe, virial [3, 3]) of npt_reference's kind with the bias added to all three (with_virial False:
    the bias virial left out, for the test that it matters)"""
    def ev(x, lo, length):
        f, pe, w = evaluate_model(x, lo, length)
        fb, eb, wb, _ = bias(x, restraints, length)
        w = np.asarray(w, dtype=np.float64)
        w = np.diag([w / 3.0] * 3) if w.ndim == 0 else w.reshape(3, 3)
        return f + fb, pe + eb, w + wb if with_virial else w
    return ev


def nve_trajectory(x0, v0, mass, evaluate_total, steps, dt):
    """velocity Verlet in the order of the loop's kernels: v += dtfm f; x += dt v; f = F(x); v += dtfm f.  evaluate_total(x) ->
    (f, pe).  Returns the records of step 0 .. steps: dicts of x, v, f, pe, ke."""
    mass = np.asarray(mass, dtype=np.float64)
    dtfm = ((0.5 * dt * FTM2V) / mass)[:, None]
    x, v = np.array(x0, dtype=np.float64), np.array(v0, dtype=np.float64)
    f, pe = evaluate_total(x)

    def record():
        return dict(x=x.copy(), v=v.copy(), f=f.copy(), pe=float(pe), ke=0.5 * MVV2E * float((mass[:, None] * v * v).sum()))

    out = [record()]
    for _ in range(steps):
        v = v + dtfm * f
        x = x + dt * v
        f, pe = evaluate_total(x)
        v = v + dtfm * f
        out.append(record())
    return out


# ---- the cases of the kernel test ---------------------------------------------------------------------------------------------
def chain_case(nr, seed, L=20.0, pmask=7, hub=False, extra=5):
    """nr consecutive restraints of mixed kinds on a random-walk chain of nr + 3 atoms (restraint i on atoms i .. i + 3 of the chain,
    kind i % 3 rotated by the seed), bond lengths in [0.9, 1.6] A, bond angles in [60, 120] degrees, free torsions; the chain starts
    0.5 A inside the +x face and is wrapped into the box of side(s) L in the periodic dimensions; `extra` atoms in no restraint; atom
    indices shuffled.  hub: the distance restraints from the fifth on (up to nine) join atom 2 of the chain to an atom further down
    instead, so that one atom collects eight or more entries.  kappa in [5, 50], centres within 0.3 of the value.
    Returns dict(x [n, 3], atoms, kind, kappa, centre, len [3], pmask, untouched: the atoms in no restraint, the `extra` ones and
    whatever the last restraint leaves of the chain's end)."""
    rng = np.random.default_rng(seed)
    nc = nr + 3
    L = np.array(np.broadcast_to(np.asarray(L, dtype=np.float64), 3))
    p = np.zeros((nc, 3))
    p[0] = (L[0] - 0.5, 0.3, 0.5 * L[2])
    d0 = rng.normal(size=3)
    p[1] = p[0] + rng.uniform(0.9, 1.6) * d0 / np.linalg.norm(d0)
    for i in range(1, nc - 1):
        e1 = (p[i - 1] - p[i]) / np.linalg.norm(p[i - 1] - p[i])
        t = rng.normal(size=3)
        t -= (t @ e1) * e1
        t /= np.linalg.norm(t)
        th = np.deg2rad(rng.uniform(60.0, 120.0))
        p[i + 1] = p[i] + rng.uniform(0.9, 1.6) * (np.cos(th) * e1 + np.sin(th) * t)
    x = np.concatenate([p, rng.uniform(0.0, L, size=(extra, 3))])
    for k in range(3):
        if (pmask >> k) & 1:
            x[:, k] = np.mod(x[:, k], L[k])
    perm = rng.permutation(nc + extra)                       # chain atom j is atom perm[j]
    xs = np.zeros_like(x)
    xs[perm] = x
    kinds = (np.arange(nr) + int(seed)) % 3
    idx = [list(range(i, i + NATOMS_OF[int(kinds[i])])) for i in range(nr)]
    if hub:
        far = [i for i in range(nr) if kinds[i] == DISTANCE and i >= 8][:9]
        for i in far:
            idx[i] = [2, i + 1]
    atoms = np.full((nr, 4), -1, dtype=np.int32)
    for i, ix in enumerate(idx):
        atoms[i, : len(ix)] = perm[ix]
    length = L
    kappa = rng.uniform(5.0, 50.0, nr)
    cv = evaluate(xs, atoms, kinds, kappa, np.zeros(nr), length, pmask)["cv"]
    centre = cv + rng.uniform(-0.3, 0.3, nr)
    return dict(x=xs, atoms=atoms, kind=kinds.astype(np.int32), kappa=kappa, centre=centre, len=length, pmask=pmask,
                untouched=np.setdiff1d(np.arange(nc + extra), atoms[atoms >= 0]))
