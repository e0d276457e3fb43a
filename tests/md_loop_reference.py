"""Plain numpy (and Python integers / fractions) forms of the time-step loop's kernels in include/ani_md.h: the integrators with
the Langevin thermostat's counter-based generator, the ghost copies and sums, gather / scatter, the position wrap, the ghost
shell (count, scan, fill, append) and the displacement check.  tests/test_md_loop_reference_cpu.py tests this file on the CPU
(the generator's moments, the thermostat's stationary temperature, the wrap, the shell); tests/test_md_loop_kernels.py compares
the kernels with it one call at a time.

Every floating-point expression is written in the kernels' operation order and evaluated WITHOUT fused multiply-adds (numpy has
none); the device may fuse each multiply-add, which is what the GPU tests' bars account for.  The wrap alone is exact: rational
arithmetic on the doubles' exact values.
"""
from fractions import Fraction

import numpy as np

MASK64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15            # the golden-ratio increment of splitmix64
C = 0xD1B54A32D192ED03            # the multiplier that spreads the tags
BLOCK = 256                       # atoms per block of the integrators and the ghost shell


# ---- the generator ----------------------------------------------------------------------------------------------------------
def mix64(z):
    """splitmix64 finaliser on uint64 with wrap-around; z: anything that converts to a uint64 array (Python ints < 2^64)"""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64)).copy()
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draws(seed, step, tags):
    """[n, 3] uniform numbers in [-0.5, 0.5) of the atoms with the global tags `tags` (int64, or anything integer) at `step`:
    key = mix64(seed + G (step + 1)) ^ (C tag),  r_k = (mix64(key + G (k + 1)) >> 11) 2^-53 - 0.5.  seed, step: Python integers,
    taken modulo 2^64 like the kernel's unsigned arguments."""
    tags = np.atleast_1d(np.asarray(tags)).astype(np.int64).astype(np.uint64)         # two's complement, as the kernel's cast
    base = mix64((int(seed) + G * (int(step) + 1)) & MASK64)[0]
    with np.errstate(over="ignore"):
        key = base ^ (np.uint64(C) * tags)
        h = np.stack([mix64(key + np.uint64((G * (k + 1)) & MASK64)) for k in range(3)], axis=1)
    # h >> 11 < 2^53 converts exactly, the scaling by a power of two is exact, and so is the subtraction (a multiple of 2^-53 of
    # magnitude at most 0.5): a draw is the same double however the device contracts the expression
    return (h >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) - 0.5


# ---- the integrators --------------------------------------------------------------------------------------------------------
def _d2(x, x_built):
    d = x - x_built
    return (0.0 + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def _fold(d2max, d2):
    return max(float(d2max), float(d2.max())) if d2.size else float(d2max)


def initial_integrate(x, v, f, dtfm, dt, x_built, d2max):
    """v += dtfm f;  x += dt v;  returns (x, v, max(d2max, |x - x_built|^2)) -- new arrays, the inputs are not written"""
    v = v + dtfm[:, None] * f
    x = x + dt * v
    return x, v, _fold(d2max, _d2(x, x_built))


def thermostat(v, f, g1, g2, tags, seed, step):
    """f + (g1 v + g2 r), r = draws(seed, step, tags); tags None: the local index"""
    r = draws(seed, step, np.arange(v.shape[0]) if tags is None else tags)
    return f + (g1[:, None] * v + g2[:, None] * r)


def final_integrate(v, f, dtfm, langevin=0, g1=None, g2=None, tags=None, seed=0, step=0):
    """langevin: f += g1 v + g2 r;  then v += dtfm f;  returns (v, f)"""
    if langevin:
        f = thermostat(v, f, g1, g2, tags, seed, step)
    return v + dtfm[:, None] * f, f


def final_initial_integrate(x, v, f, dtfm, dt, x_built, d2max, langevin=0, g1=None, g2=None, tags=None, seed=0, step=0):
    """final_integrate of the step that ends, then initial_integrate of the step that begins; returns (x, v, f, d2max)"""
    v, f = final_integrate(v, f, dtfm, langevin, g1, g2, tags, seed, step)
    x, v, d2max = initial_integrate(x, v, f, dtfm, dt, x_built, d2max)
    return x, v, f, d2max


# ---- the ghost operations (every one returns a new array) ------------------------------------------------------------------
def forward(x, owner, shift, nlocal):
    """x[nlocal + g] = x[owner[g]] + shift[g]"""
    x = x.copy()
    ng = len(owner)
    x[nlocal:nlocal + ng] = x[owner] + shift[:ng]
    return x


def pack(x, owner, shift):
    """out[s] = x[owner[s]] + shift[s]"""
    return x[owner] + shift[:len(owner)]


def unpack_reverse(f, owner, inp):
    """f[owner[s]] += in[s]"""
    f = f.copy()
    np.add.at(f, owner, inp[:len(owner)])
    return f


def reverse(f, owner, nlocal):
    """f[owner[g]] += f[nlocal + g]"""
    return unpack_reverse(f, owner, f[nlocal:nlocal + len(owner)])


def reverse_ordered(f, owner, ghost_of, nlocal):
    """f[owner[g]] += f[nlocal + ghost_of[g]]  (ghost_of None: reverse)"""
    if ghost_of is None:
        return reverse(f, owner, nlocal)
    return unpack_reverse(f, owner, f[nlocal + np.asarray(ghost_of)])


def gather(src, idx):
    """out[k] = src[idx[k]]"""
    return src[idx].copy()


def scatter(dst, idx, inp):
    """dst[idx[k]] = in[k]"""
    dst = dst.copy()
    dst[idx] = inp[:len(idx)]
    return dst


def append(x, species, nlocal, owner, shift):
    """x[nlocal + g] = x[owner[g]] + shift[g],  species[nlocal + g] = species[owner[g]];  returns (x, species)"""
    x, species = forward(x, owner, shift, nlocal), species.copy()
    species[nlocal:nlocal + len(owner)] = species[owner]
    return x, species


# ---- the wrap ---------------------------------------------------------------------------------------------------------------
def wrap_exact(v, lo, L):
    """The true representative of the double v in [lo, lo + L), as a Fraction: t = v - floor((v - lo) / L) L in exact rational
    arithmetic on the exact values of the three doubles."""
    v, lo, L = Fraction(float(v)), Fraction(float(lo)), Fraction(float(L))
    q = (v - lo) / L
    t = v - (q.numerator // q.denominator) * L
    assert lo <= t < lo + L
    return t


def wrap_plain(v, lo, L):
    """The loop's formula in plain double precision, without a fused multiply-add and WITHOUT the clamp at the lower face:
    v -= floor((v - lo) / L) L;  if (v >= lo + L) v = lo.  Kept as the record of why the clamp exists: it can return a value
    below lo (tests/test_md_loop_reference_cpu.py)."""
    v = np.asarray(v, dtype=np.float64)
    out = v - np.floor((v - lo) / L) * L
    return np.where(out >= lo + L, lo, out)


def wrap_fixed(v, lo, L):
    """wrap_plain with the clamp of wrap_kernel and comm.DomainComm.exchange: a result below lo becomes lo"""
    out = wrap_plain(v, lo, L)
    return np.where(out < lo, lo, out)


# ---- the ghost shell --------------------------------------------------------------------------------------------------------
def shell(x, clo, chi, cshift):
    """Atom a is a ghost of combination c when clo[c] <= x[a] < chi[c] in all three dimensions.  Returns
    (blk_cnt [ncombo * nblk], blk_off [ncombo * nblk], out_counts [1 + ncombo], send_idx [hits], send_shift [hits, 3],
    ghosts [hits, 3] = x[send_idx] + send_shift): hits per (combination, block of 256 atoms), their exclusive scan, the total and
    the hits per combination, and the hits themselves combination-major with atoms ascending.  nblk = ceil(n / 256), at least 1."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    clo, chi, cshift = (np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in (clo, chi, cshift))
    n, ncombo = x.shape[0], clo.shape[0]
    nblk = max((n + BLOCK - 1) // BLOCK, 1)
    c, a = ((x[None, :, :] >= clo[:, None, :]) & (x[None, :, :] < chi[:, None, :])).all(-1).nonzero()
    blk_cnt = np.zeros(ncombo * nblk, dtype=np.int64)
    np.add.at(blk_cnt, c * nblk + a // BLOCK, 1)
    blk_off = np.cumsum(blk_cnt) - blk_cnt
    out_counts = np.concatenate([[len(a)], np.bincount(c, minlength=ncombo)]).astype(np.int64)
    send_shift = cshift[c]
    return (blk_cnt.astype(np.int32), blk_off.astype(np.int32), out_counts.astype(np.int32), a.astype(np.int64), send_shift,
            x[a] + send_shift)


# ---- the check --------------------------------------------------------------------------------------------------------------
def check(d2max, e):
    """(out, d2max after): out = d2max, or +inf when the energy e is not finite; the running maximum is zeroed either way"""
    return (float(d2max) if np.isfinite(e) else float("inf")), 0.0
