"""Inputs, references and bars of the AEV-stage edge tests (tests/test_aev_edges_cpu.py, tests/test_aev_edges.py).  No GPU.

What picks an AEV kernel (``fast_plan()`` in ani_aev_launch.h, read by ``launch_nbr_compact`` in ani_kernels_aev_lists.hip and by
``launch_aev_forward``, ``launch_aev_forward_fused``, ``launch_aev_backward`` in ani_kernels_aev_fast.hip): the model shape (8x4, 4x8,
generic), ``compat``, the longest candidate list (<= 128, <= 192, <= 256, more),
the width of the pruned AEV row (<= 256 floats or more) and the virial flag; the per-centre lists sit in LDS behind two
capacities, ``kMaxAng`` = 96 and ``radial_cap()`` = 3/4 of the longest list, at least 128, in steps of 64 (the whole list in
compat mode).  The cases here are each the smallest input that reaches one of those edges.

List cutoffs.  ``harness.decompose(system, cutoff=c, skin=0)`` with c >= Rcr is a legitimate list; c is chosen so that the
longest list has EXACTLY the length a case is named for.  The values in ``CUTOFF`` are the midpoints of the interval of c that
gives that length (bisected once; the intervals are at least 1.5e-4 A wide, the values carry six decimals), and ``build_input``
asserts the resulting maximum.

List form.  The library sorts every candidate list stably by neighbour species when it installs it, so the last candidate
of a row is the last entry of its highest species.  ``strong_last`` moves the NEAREST neighbour of every row's highest neighbour
species to the end of its segment: entry ``numneigh - 1`` is then a strong contributor of every row, and entry 128, 192 or 256 of the
longest row -- the first one of a further 64-entry chunk -- is one whose loss shows (``boundary_mutations`` and the CPU module
prove it on the reference alone).  ``shuffled`` is the same list with every segment in random order.

Bars.  Per case and ``radial_compat``: e32 = the error of the fp32 build of the oracle against the fp64 build, in the max norm,
for the AEV rows, and for the forces and the virial of ``Oracle.aev_vjp`` fed the fp64 oracle's own dE/dAEV.  bar = min(MARGIN *
e32, cap), the caps being the project's tolerances (1e-5 * max(1, largest AEV entry) as in test_hip_aev_matches_oracle; F_TOL;
V_TOL * max(1, nlocal / 100)).  The code under test never enters its own bar.  MARGIN = 8 over an fp32 evaluation with libm:
the kernels use the hardware's exp / cos / rsqrt (1 to 2 ulp against 0.5), the backward kernel takes its sixteen radial Gaussians
from two exponentials by recurrence, ``fast_kind`` parameter sets let terms below e^-20 of a row's largest go, and the force sums
are atomics in arbitrary order.
"""
from __future__ import annotations

import dataclasses
import functools
import os

import numpy as np

import list_forms as lf
from lammps_ani_amd import harness as hx, model_file as mf
from test_hip_parity import F_TOL, V_TOL

K_MAX_ANG = 96      # ani_kernels.h: kMaxAng
K_MAX_RAD = 256     # ani_kernels.h: kMaxRad (generic and fp64 kernels)
MARGIN = 8.0
AEV_CAP = 1e-5      # x max(1, largest entry): test_hip_aev_matches_oracle
MODEL_SEED = 2024
SHUFFLE_SEED = 20250107
RCA = 3.5
RCR_ANI2X = 5.1


def radial_cap(max_numneigh, compat):
    """ani_aev_launch.h, radial_cap(): slots of the per-centre radial list"""
    full = max(64, -(-max_numneigh // 64) * 64)
    if compat:
        return full
    est = max(128, (3 * max_numneigh + 3) // 4)
    return min(-(-est // 64) * 64, full)


# ---- systems ------------------------------------------------------------------------------------------------------------

# (box, longest list) -> list cutoff in A (skin 0)
CUTOFF = {
    ("dense7", 128): 5.337748, ("dense7", 129): 5.356593, ("dense7", 192): 6.130776, ("dense7", 193): 6.132009,
    ("dense7", 256): 6.787227, ("dense7", 257): 6.799437,
    ("dense4", 129): 5.276620, ("dense4", 193): 6.140357, ("dense4", 257): 6.765512,
    ("sparse7", 193): 7.785461,
    ("water", 129): 6.531884, ("water", 193): 7.451852,
    ("dense3", 129): 5.397996, ("dense3", 257): 6.890814,
}


@functools.lru_cache(maxsize=None)
def box(name):
    if name == "dense7":
        return hx.random_box(600, 7, 15.0, seed=5)
    if name == "dense4":
        return hx.random_box(500, 4, 14.0, seed=5)
    if name == "sparse7":
        return hx.random_box(300, 7, 15.0, seed=5)
    if name == "dense3":
        return hx.random_box(300, 3, 12.0, seed=5)
    if name == "water":
        return hx.water_box(600)
    raise KeyError(name)


SHELLS = ((3.2, 0.2), (4.6, 0.4), (6.2, 0.8))   # radius, jitter of the three shells of shell_cluster
SHELL_LIST_CUTOFF = 7.1


def _fibonacci_sphere(n, phase):
    k = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * k / n)
    th = np.pi * (1 + 5 ** 0.5) * k + phase
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)


def shell_cluster(counts, ntypes=7, seed=5):
    """Open boundaries: atom 0 at the origin and ``counts`` atoms on three Fibonacci spheres around it, at 3.2 +- 0.2 A (inside
    Rca), 4.6 +- 0.4 A (between Rca and Rcr) and 6.2 +- 0.8 A (beyond Rcr, inside a 7.1 A list); types random in 1..ntypes."""
    rng = np.random.default_rng(seed)
    pts = [np.zeros((1, 3))]
    for n, (r, dr) in zip(counts, SHELLS):
        if n:
            pts.append(_fibonacci_sphere(n, rng.uniform(0, 2 * np.pi)) * (r + rng.uniform(-dr, dr, size=(n, 1))))
    x = np.concatenate(pts)
    t = rng.integers(1, ntypes + 1, size=len(x)).astype(np.int32)
    return hx.System(x, t, np.full(3, -30.0), np.full(3, 30.0), (False, False, False))


# atom indices of the centres of interest in the degenerate input
DEGENERATE = dict(empty=0, single=1, two=3, radial_only=6)


def degenerate_system():
    """Open boundaries, groups 30 A apart: an atom alone; a pair 2.0 A apart (one neighbour inside Rca each: no angular pair); an
    atom with exactly two neighbours inside Rca, 2.5 A away on opposite sides (they see each other at 5.0 A, between Rca and Rcr);
    a pair 4.2 A apart (only a radial-only neighbour); and a 22-atom cluster, which makes 30 centres (not a multiple of 4: the
    forward and backward kernels take four centres per workgroup)."""
    x = [[0.0, 0, 0],
         [30.0, 0, 0], [32.0, 0, 0],
         [60.0, 0, 0], [62.5, 0, 0], [57.5, 0, 0],
         [90.0, 0, 0], [94.2, 0, 0]]
    t = [1, 4, 1, 2, 1, 6, 5, 7]
    c = hx.random_box(22, 7, 6.5, seed=3, min_dist=1.0)
    x = np.concatenate([np.array(x), c.x + np.array([0.0, 40.0, 0.0])])
    t = np.concatenate([np.array(t, np.int32), c.types])
    return hx.System(x, t.astype(np.int32), np.full(3, -20.0), np.full(3, 120.0), (False, False, False))


# ---- cases ----------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Case:
    model: str                  # "ani2x", "ani1x", "tiny" or "ani2x-eta80"
    kernels: str                # "8x4", "4x8" or "generic": the instantiation family
    box: str = ""               # a box of box(), listed at CUTOFF[(box, longest)]
    longest: int = 0            # numneigh.max(), asserted
    shell: tuple = ()           # or: the counts of a shell_cluster
    shell_seed: int = 5
    boundaries: tuple = ()      # the chunk bounds b the case is named for (see boundary_mutations)
    within: tuple = ()          # (max inside Rcr, max inside Rca, max between) over the centres, asserted


def _named(longest):
    return (longest if longest % 64 == 0 else longest - 1,)


CASES = {}
for _n in (128, 129, 192, 193, 256, 257):
    CASES[f"dense7-{_n}"] = Case("ani2x", "8x4", "dense7", _n, boundaries=_named(_n), within=(115, 43, 82))
CASES["sparse7-193"] = Case("ani2x", "8x4", "sparse7", 193, boundaries=(192,), within=(61, 25, 45))
for _n in (129, 193, 257):
    CASES[f"dense4-{_n}"] = Case("ani1x", "4x8", "dense4", _n, boundaries=_named(_n), within=(124, 43, 94))
for _n in (129, 193):
    CASES[f"water-{_n}"] = Case("ani2x", "8x4", "water", _n, boundaries=_named(_n), within=(66, 25, 52))
# the centre's list has 256 entries, 96 of them inside Rca and 192 inside Rcr: kMaxAng and radial_cap(256) = 192 met exactly; with
# use_cuaev = False (the issue's shell-full-compat) the capacity is the list length, met exactly too
CASES["shell-full"] = Case("ani2x", "8x4", shell=(96, 96, 64), longest=256, boundaries=(256,))
for _n in (129, 257):
    CASES[f"generic-tiny-{_n}"] = Case("tiny", "generic", "dense3", _n, boundaries=_named(_n), within=(111, 41, 84))
    CASES[f"generic-eta80-{_n}"] = Case("ani2x-eta80", "generic", "dense7", _n, boundaries=_named(_n), within=(115, 43, 82))
# the generic kernels' lists: kMaxRad = 256 entries inside Rcr and kMaxAng = 96 inside Rca, both met exactly by the centre
CASES["generic-shell-full"] = Case("ani2x-eta80", "generic", shell=(96, 160, 0), shell_seed=2, longest=256, boundaries=(256,))
CASES["degenerate"] = Case("ani2x", "8x4")
CASE_IDS = tuple(CASES)

# one atom more than a capacity holds: (counts, seed, model, what the centre then has inside Rca / inside Rcr)
OVER = {
    "shell-angular-97": dict(shell=(97, 95, 64), seed=5, model="ani2x", ang=97, rad=192),
    "shell-radial-193": dict(shell=(96, 97, 63), seed=5, model="ani2x", ang=96, rad=193),
    "generic-shell-radial-257": dict(shell=(96, 161, 0), seed=2, model="ani2x-eta80", ang=96, rad=257),
}


def model_path(model, model_cache, members=2):
    """the model file of a case: the session's synthetic models; "ani2x-eta80" is the ANI-2x shape with EtaR = 80, which
    ``fast_kind`` sends to the generic kernels (test_hip_radial_widths_other_than_the_published_ones: beyond-the-guard)"""
    if model != "ani2x-eta80":
        return model_cache(model, members, MODEL_SEED)
    base = model_cache("ani2x", members, MODEL_SEED)
    p = base[: -len(".anim")] + "_eta80.anim"
    if not os.path.exists(p):
        m = mf.synthetic_model("ani2x", members, MODEL_SEED)
        m.EtaR = 80.0
        mf.write_model(p, m)
    return p


def rcr_of(model):
    return 5.2 if model == "ani1x" else RCR_ANI2X


# ---- list forms -------------------------------------------------------------------------------------------------------------

def strong_last(inp):
    """every segment with the nearest neighbour of the row's highest neighbour species moved to its end (module docstring)"""
    assert not inp.half
    off = lf._offsets(inp.numneigh)
    jl = inp.jlist.copy()
    for k in range(inp.nlocal):
        a, b = int(off[k]), int(off[k + 1])
        if b - a < 2:
            continue
        seg = inp.jlist[a:b]
        d = inp.x[seg] - inp.x[inp.ilist[k]]
        r2 = np.einsum("ij,ij->i", d, d)
        t = inp.types[seg]
        cand = np.nonzero(t == t.max())[0]
        pick = int(cand[np.argmin(r2[cand])])
        jl[a:b] = np.concatenate([np.delete(seg, pick), seg[pick: pick + 1]])
    return dataclasses.replace(inp, jlist=jl)


def installed_order(inp, k):
    """segment k as the library installs it: sorted stably by neighbour species"""
    seg = lf.segments(inp)[k]
    return seg[np.argsort(inp.types[seg], kind="stable")]


@functools.lru_cache(maxsize=None)
def build_input(name):
    """the strong-last full list of case (or over-capacity input) ``name``; cached, treat as read-only"""
    if name in OVER:
        o = OVER[name]
        return strong_last(hx.decompose(shell_cluster(o["shell"], seed=o["seed"]), cutoff=SHELL_LIST_CUTOFF, skin=0.0))
    c = CASES[name]
    if name == "degenerate":
        return strong_last(hx.decompose(degenerate_system()))
    if c.shell:
        inp = hx.decompose(shell_cluster(c.shell, seed=c.shell_seed), cutoff=SHELL_LIST_CUTOFF, skin=0.0)
    else:
        inp = hx.decompose(box(c.box), cutoff=CUTOFF[(c.box, c.longest)], skin=0.0)
    assert int(inp.numneigh.max()) == c.longest, (name, int(inp.numneigh.max()))
    return strong_last(inp)


@functools.lru_cache(maxsize=None)
def shuffled(name):
    return lf.shuffle_segments(build_input(name), np.random.default_rng(SHUFFLE_SEED))


@functools.lru_cache(maxsize=None)
def half_input(name):
    """the half list of the same pairs (boxes only); the library forms the per-centre lists itself"""
    c = CASES[name]
    return hx.decompose(box(c.box), cutoff=CUTOFF[(c.box, c.longest)], skin=0.0, half=True)


def counts(inp, rcr):
    """per centre: entries inside Rcr, inside Rca, between the two"""
    r, a = lf.neighbours_within(inp, rcr), lf.neighbours_within(inp, RCA)
    return r, a, r - a


def min_distance(system):
    x = system.x
    d = x[:, None, :] - x[None, :, :]
    r2 = np.einsum("ijk,ijk->ij", d, d) + np.eye(len(x)) * 1e9
    return float(np.sqrt(r2.min()))


# ---- references and bars ------------------------------------------------------------------------------------------------------

_REFS = {}


def reference(name, compat, path):
    """fp64 oracle results of case ``name`` (strong-last list), the fp32 build's distance from them, and the bars.  Cached per
    (case, compat): dict(aev, gaev, force, virial [fp64 oracle], e32 = dict(aev, force, virial), bar = the same keys)."""
    from oracle import Oracle
    key = (name, bool(compat), path)
    if key not in _REFS:
        inp = build_input(name)
        o64 = Oracle(path).compute(inp, radial_compat=compat, want_aev=True)
        o32 = Oracle(path, fp32=True)
        a32 = o32.compute(inp, radial_compat=compat, want_aev=True)["aev"]
        v32 = o32.aev_vjp(inp, o64["gaev"], radial_compat=compat)
        e32 = dict(aev=float(np.abs(a32.astype(np.float64) - o64["aev"]).max()),
                   force=float(np.abs(v32["force"] - o64["force"]).max()),
                   virial=float(np.abs(v32["virial"] - o64["virial"]).max()))
        cap = dict(aev=AEV_CAP * max(1.0, float(np.abs(o64["aev"]).max())), force=F_TOL, virial=V_TOL * max(1.0, inp.nlocal / 100.0))
        bar = {k: min(MARGIN * e32[k], cap[k]) for k in e32}
        _REFS[key] = dict(aev=o64["aev"], gaev=o64["gaev"], force=o64["force"], virial=o64["virial"], energy=o64["energy"],
                          e32=e32, cap=cap, bar=bar, fp32=dict(aev=a32, force=v32["force"], virial=v32["virial"]))
    return _REFS[key]


def bars(ref, margin=MARGIN):
    """the bars of a reference() at another margin (a path whose margin was raised, never past the caps)"""
    return {k: min(margin * ref["e32"][k], ref["cap"][k]) for k in ref["e32"]}


# ---- teeth: what losing or doubling the boundary entry does to the reference ----------------------------------------------------

def _one_centre(inp, k, seg):
    """the input reduced to centre k with the segment ``seg``: the oracle then returns this centre's AEV row and its part of
    the forces (every other atom is a 'ghost' of the reduced input)"""
    return dataclasses.replace(inp, nlocal=1, nghost=inp.ntotal - 1, ilist=inp.ilist[k: k + 1].astype(np.int32),
                               numneigh=np.array([len(seg)], np.int32), jlist=np.asarray(seg, np.int32),
                               owner_rank=np.zeros(inp.ntotal - 1, np.int32), owner_lidx=np.zeros(inp.ntotal - 1, np.int32),
                               shift=np.zeros((inp.ntotal - 1, 3), np.int32))


def boundary_positions(name):
    """[(centre k, position p in the installed order)]: for every bound b the case is named for, the entry that sits on it in
    every longest row -- position b - 1 where the longest list has b entries (the last one of a full chunk), position b where
    it has b + 1 (the first and only one of a further chunk).  With strong_last both are the row's last entry."""
    c, inp = CASES[name], build_input(name)
    out = []
    for b in c.boundaries:
        p = b - 1 if c.longest == b else b
        rows = np.nonzero(inp.numneigh > p)[0]
        assert rows.size > 0 and p == c.longest - 1, (name, b)
        out += [(int(k), p) for k in rows]
    if c.shell:
        # the centre of a shell cluster fills both LDS streams exactly: also the last entry of its angular stream (inside Rca) and
        # the last one of its radial-only stream (between Rca and Rcr), the entries a capacity off by one would drop
        seg = installed_order(inp, 0)
        r = np.linalg.norm(inp.x[seg] - inp.x[inp.ilist[0]], axis=1)
        ends = [int(np.nonzero(r <= RCA)[0][-1]), int(np.nonzero((r > RCA) & (r <= rcr_of(c.model)))[0][-1])]
        out += [(0, p) for p in ends if (0, p) not in out]
    return out


def boundary_mutations(name, compat, path, ref):
    """For each boundary entry: the max-norm change of the fp64 AEV row and of the fp64 aev_vjp forces when the entry is removed
    from its row, and when it is there twice.  Yields (centre, position, "removed" | "doubled", d_aev, d_force)."""
    from oracle import Oracle
    inp = build_input(name)
    o = Oracle(path)
    for k, p in boundary_positions(name):
        seg = installed_order(inp, k)
        g = ref["gaev"][k: k + 1]
        base = _one_centre(inp, k, seg)
        a0 = o.compute(base, radial_compat=compat, want_aev=True)["aev"]
        assert np.abs(a0[0] - ref["aev"][k]).max() < 1e-12
        f0 = o.aev_vjp(base, g, radial_compat=compat)["force"]
        for what, mut in (("removed", np.delete(seg, p)), ("doubled", np.insert(seg, p, seg[p]))):
            m = _one_centre(inp, k, mut)
            a1 = o.compute(m, radial_compat=compat, want_aev=True)["aev"]
            f1 = o.aev_vjp(m, g, radial_compat=compat)["force"]
            yield k, p, what, float(np.abs(a1 - a0).max()), float(np.abs(f1 - f0).max())
