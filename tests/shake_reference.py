"""numpy fp64 RATTLE, written from the contract of ani_md_shake_positions / ani_md_rattle_velocities in include/ani_md.h (Andersen
1983; LAMMPS `fix shake` / `fix rattle` on clusters of a centre and one to three partners): the reference of every constraint test.

`build_clusters` applies the rules of `lammps_ani_amd.md.constraint_clusters` (written independently: a graph walk over the
components); `shake_positions` is the position stage by Newton to 1e-15 or 60 iterations, `rattle_velocities` the velocity stage
by `np.linalg.solve`.  `kernel_case(nc)` is the input recipe of tests/test_shake_kernels.py, defined here once and validated on the
CPU by tests/test_shake_reference_cpu.py; its reference results are computed once per session (`kernel_case_reference`).
"""
import functools

import numpy as np

FTM2V = 1.0 / 48.88821291 / 48.88821291   # LAMMPS units real, as lammps_ani_amd.md
MVV2E = 48.88821291 * 48.88821291
BOLTZ = 0.0019872067
MASSES = np.array([1.008, 12.011, 14.007, 15.999, 32.06, 18.998, 35.45])
BOND_LENGTHS = (0.96, 1.09, 1.01)          # O-H, C-H, N-H of the reference's alanine-dipeptide data file, in A


def minimg(a, L, periodic=(True, True, True)):
    a = np.array(a, dtype=np.float64)
    for k in range(3):
        if periodic[k]:
            a[..., k] -= L[k] * np.round(a[..., k] / L[k])
    return a


def build_clusters(bonds, tags):
    """(cl [nc, 4] int32, slot_bond [nc, 3] int64) like lammps_ani_amd.md.constraint_clusters, by walking the components"""
    bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    tags = [int(t) for t in np.asarray(tags).reshape(-1)]
    where = {}
    for i, t in enumerate(tags):
        where[t] = i
    adj = {}
    pairs = set()
    for b, (ta, tb) in enumerate(bonds.tolist()):
        if ta not in where:
            raise ValueError(f"unknown tag {ta}")
        if tb not in where:
            raise ValueError(f"unknown tag {tb}")
        if ta == tb:
            raise ValueError(f"self-bond on tag {ta}")
        if frozenset((ta, tb)) in pairs:
            raise ValueError(f"duplicate bond between tags {ta} and {tb}")
        pairs.add(frozenset((ta, tb)))
        adj.setdefault(where[ta], {})[where[tb]] = b
        adj.setdefault(where[tb], {})[where[ta]] = b
    done, out = set(), []
    for start in sorted(adj):
        if start in done:
            continue
        comp, stack = [], [start]
        done.add(start)
        while stack:
            i = stack.pop()
            comp.append(i)
            for j in adj[i]:
                if j not in done:
                    done.add(j)
                    stack.append(j)
        nbonds = sum(len(adj[i]) for i in comp) // 2
        hubs = [i for i in comp if len(adj[i]) > 1]
        if len(comp) == 2:
            centre = min(comp)
        elif len(hubs) == 1 and nbonds == len(comp) - 1 and len(adj[hubs[0]]) == len(comp) - 1:
            centre = hubs[0]
        else:
            raise ValueError(f"the component of tag {tags[hubs[0]]} is not a star")
        if len(adj[centre]) > 3:
            raise ValueError(f"tag {tags[centre]} has {len(adj[centre])} partners")
        out.append((centre, sorted(adj[centre].items())))
    out.sort(key=lambda c: (len(c[1]), c[0]))
    cl = np.full((len(out), 4), -1, dtype=np.int32)
    slot_bond = np.full((len(out), 3), -1, dtype=np.int64)
    for c, (i, nb) in enumerate(out):
        cl[c, 0] = i
        for k, (j, b) in enumerate(nb):
            cl[c, 1 + k], slot_bond[c, k] = j, b
    return cl, slot_bond


def canonical(cl):
    """cluster table as a set of (centre, partners) with the two atoms of a two-atom cluster in either order"""
    out = set()
    for row in np.asarray(cl).tolist():
        p = tuple(sorted(j for j in row[1:] if j >= 0))
        out.add((min(row[0], p[0]), (max(row[0], p[0]),)) if len(p) == 1 else (row[0], p))
    return out


def residuals(x, cl, d, L, periodic=(True, True, True)):
    """| |r_k|^2 - d_k^2 | / d_k^2 of every used slot, [nc, 3] (0 in unused slots)"""
    cl, d = np.asarray(cl), np.asarray(d, dtype=np.float64)
    out = np.zeros(d.shape)
    for k in range(3):
        u = cl[:, 1 + k] >= 0
        r = minimg(x[cl[u, 0]] - x[cl[u, 1 + k]], L, periodic)
        out[u, k] = np.abs((r * r).sum(1) - d[u, k] ** 2) / d[u, k] ** 2
    return out


def shake_positions(x, v, cl, d, w, dt, L, periodic=(True, True, True), tol=1e-15, maxiter=60):
    """Position stage on copies: x holds x', v the half-step velocity (None: x0 = x', no velocity).  Returns (x, v, iterations [nc],
    final relative residual [nc])."""
    x = np.array(x, dtype=np.float64)
    xin = x.copy()
    vout = None if v is None else np.array(v, dtype=np.float64)
    x0 = x if v is None else x - dt * vout
    nc = len(cl)
    iters, res = np.zeros(nc, dtype=np.int64), np.zeros(nc)
    for c in range(nc):
        ic = int(cl[c][0])
        ip = [int(j) for j in cl[c][1:] if j >= 0]
        K = len(ip)
        dd = np.asarray(d[c][:K], dtype=np.float64) ** 2
        s = minimg(x0[ic] - x0[ip], L, periodic)              # [K, 3]
        rp = minimg(xin[ic] - xin[ip], L, periodic)
        wc, wp = w[ic], w[ip]
        g = np.zeros(K)
        while True:
            r = rp + wc * (g @ s) + (wp * g)[:, None] * s
            F = (r * r).sum(1) - dd
            res[c] = np.abs(F / dd).max()
            if (np.abs(F) <= tol * dd).all() or iters[c] == maxiter:
                break
            J = 2.0 * (r @ s.T) * (wc + np.diag(wp))
            g = g + np.linalg.solve(J, -F)
            iters[c] += 1
        dxc = wc * (g @ s)
        dxp = -(wp * g)[:, None] * s
        x[ic] = xin[ic] + dxc
        x[ip] = xin[ip] + dxp
        if vout is not None:
            vout[ic] += dxc / dt
            vout[ip] += dxp / dt
    return x, vout, iters, res


def rattle_velocities(x, v, cl, w, L, periodic=(True, True, True)):
    """Velocity stage on a copy of v: r_k . (v_c - v_pk) = 0 for every constrained bond"""
    v = np.array(v, dtype=np.float64)
    for c in range(len(cl)):
        ic = int(cl[c][0])
        ip = [int(j) for j in cl[c][1:] if j >= 0]
        r = minimg(x[ic] - x[ip], L, periodic)
        wc, wp = w[ic], w[ip]
        A = wc * (r @ r.T) + np.diag(wp * (r * r).sum(1))
        h = np.linalg.solve(A, -(r * (v[ic] - v[ip])).sum(1))
        v[ic] += wc * (h @ r)
        v[ip] -= (wp * h)[:, None] * r
    return v


def velocity_defect(x, v, cl, L, periodic=(True, True, True)):
    """largest |r_k . (v_c - v_pk)| / |r_k| over the used slots"""
    worst = 0.0
    for k in range(3):
        u = cl[:, 1 + k] >= 0
        if u.any():
            r = minimg(x[cl[u, 0]] - x[cl[u, 1 + k]], L, periodic)
            dv = v[cl[u, 0]] - v[cl[u, 1 + k]]
            worst = max(worst, float((np.abs((r * dv).sum(1)) / np.sqrt((r * r).sum(1))).max()))
    return worst


# ---- the input recipe of tests/test_shake_kernels.py ---------------------------------------------------------------------
KERNEL_COUNTS = [1, 63, 64, 65, 255, 256, 257, 1500]     # a lone thread, wave edges, block edges, several blocks
BOX, DT, SIGMA_V = 20.0, 2.0, 0.05


def _directions(rng, K, first=None):
    """K unit vectors, every pair at least 60 degrees apart (first: the first one, given)"""
    while True:
        u = rng.normal(size=(K, 3))
        u /= np.sqrt((u * u).sum(1))[:, None]
        if first is not None:
            u[0] = first
        if K == 1 or (u @ u.T)[np.triu_indices(K, 1)].max() <= 0.5:
            return u


def kernel_case(nc, seed=0):
    """dict: L [3], x0 (wrapped start, on the constraints), v, xp = x0 + dt v, cl [nc, 4] int32 (K in random order), d [nc, 3],
    w = 1 / mass [n], free (indices of the atoms in no cluster), straddling (clusters whose raw bond exceeds half the box)"""
    rng = np.random.default_rng(7000 + 13 * seed + nc)
    L = np.array([BOX, BOX, BOX])
    Ks = rng.integers(1, 4, nc)
    nbound = int(nc + Ks.sum())
    nfree = max(1, nbound // 4)
    n = nbound + nfree
    order = rng.permutation(n)                      # the clusters' atoms lie scattered through the arrays
    x0, m = np.zeros((n, 3)), np.zeros(n)
    cl, d = np.full((nc, 4), -1, dtype=np.int32), np.zeros((nc, 3))
    at = 0
    for c in range(nc):
        K = int(Ks[c])
        ic, ip = order[at], order[at + 1: at + 1 + K]
        at += 1 + K
        centre = rng.uniform(0.0, BOX, 3)
        dk = rng.choice(BOND_LENGTHS, K)
        if c == 0:                                  # placed by hand: the first bond of cluster 0 crosses the +x face
            centre[0] = BOX - 0.2
            u = _directions(rng, K, first=(1.0, 0.0, 0.0))
        else:
            u = _directions(rng, K)
        x0[ic], x0[ip] = centre, centre + dk[:, None] * u
        m[ic], m[ip] = MASSES[rng.integers(1, 4)], MASSES[0]
        cl[c, 0], cl[c, 1: 1 + K], d[c, :K] = ic, ip, dk
    free = order[at:]
    x0[free] = rng.uniform(0.0, BOX, (nfree, 3))
    m[free] = MASSES[rng.integers(0, 4, nfree)]
    x0 -= np.floor(x0 / BOX) * BOX
    x0[x0 >= BOX] = 0.0
    straddling = [c for c in range(nc) for k in range(3)
                  if cl[c, 1 + k] >= 0 and np.abs(x0[cl[c, 0]] - x0[cl[c, 1 + k]]).max() > 0.5 * BOX]
    v = rng.normal(0.0, SIGMA_V, (n, 3))
    return dict(L=L, x0=x0, v=v, xp=x0 + DT * v, cl=cl, d=d, w=1.0 / m, m=m, free=np.sort(free), straddling=sorted(set(straddling)),
                moved=np.sort(order[:at]))


@functools.lru_cache(maxsize=None)
def kernel_case_reference(nc, seed=0):
    """(case, x_ref, v_ref, iterations, v_rattled): the position stage of the case to 1e-15 and the velocity stage on its result"""
    case = kernel_case(nc, seed)
    x, v, it, res = shake_positions(case["xp"], case["v"], case["cl"], case["d"], case["w"], DT, case["L"])
    vr = rattle_velocities(x, v, case["cl"], case["w"], case["L"])
    for a in (x, v, it, vr):
        a.setflags(write=False)
    return case, x, v, it, vr


# ---- water boxes: the O-H bonds, and the oracle-driven RATTLE integrator of tests/test_shake_md.py -------------------------
def water_oh_bonds(sysm, type_H=1, type_O=4, rmax=1.3):
    """[nb, 2] (O, H) global indices: every hydrogen with its nearest oxygen (minimum image), which has to lie within rmax"""
    from scipy.spatial import cKDTree
    L = sysm.boxhi - sysm.boxlo
    xw = np.mod(sysm.x - sysm.boxlo, L)
    xw[xw >= L] = 0.0
    io, ih = np.nonzero(sysm.types == type_O)[0], np.nonzero(sysm.types == type_H)[0]
    dist, j = cKDTree(xw[io], boxsize=L).query(xw[ih])
    assert (dist < rmax).all()
    return np.stack([io[j], ih], 1).astype(np.int64)


def rattle_trajectory(sysm, bonds, v0, evaluate, steps, dt):
    """numpy velocity Verlet with RATTLE (LAMMPS fix nve order, the two stages behind its halves): bonds held at their start
    lengths, v0 projected first.  evaluate(x) -> forces [n, 3] in global order.  Returns the records of step 0 .. steps:
    dicts of x, v, f, T (3 N - 3 - nb degrees of freedom)."""
    n, L = sysm.natoms, sysm.boxhi - sysm.boxlo
    m = MASSES[sysm.types - 1]
    w = 1.0 / m
    cl, slot = build_clusters(bonds, np.arange(n))
    d = np.zeros((len(cl), 3))
    for k in range(3):
        u = cl[:, 1 + k] >= 0
        r = minimg(sysm.x[cl[u, 0]] - sysm.x[cl[u, 1 + k]], L)
        d[u, k] = np.sqrt((r * r).sum(1))
    x = sysm.x.copy()
    v = rattle_velocities(x, v0, cl, w, L)
    dof = 3.0 * n - 3.0 - len(bonds)

    def record(f):
        ke = 0.5 * MVV2E * float((m[:, None] * v * v).sum())
        return dict(x=x.copy(), v=v.copy(), f=f.copy(), T=2.0 * ke / (dof * BOLTZ))

    f = evaluate(x)
    out = [record(f)]
    for _ in range(steps):
        v = v + 0.5 * dt * FTM2V * f / m[:, None]
        x = x + dt * v
        x, v, _, _ = shake_positions(x, v, cl, d, w, dt, L)
        f = evaluate(x)
        v = v + 0.5 * dt * FTM2V * f / m[:, None]
        v = rattle_velocities(x, v, cl, w, L)
        out.append(record(f))
    return out, cl, d
