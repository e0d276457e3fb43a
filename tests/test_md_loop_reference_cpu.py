"""CPU: the numpy reference of the time-step loop's kernels (tests/md_loop_reference.py).  Runs none of the device code.  The
statistics of the Langevin thermostat are asserted HERE, on the reference; tests/test_md_loop_kernels.py then compares the
kernels with the reference deterministically."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import md_loop_reference as mr

EDGE_WORDS = (0, 1 << 63, (1 << 64) - 1)          # seed and step values at the ends of the unsigned range


@pytest.fixture(scope="module")
def sample():
    """16 steps x 4096 tags x 3 components with seed 12345: [16, 4096, 3]"""
    return np.stack([mr.draws(12345, s, np.arange(4096)) for s in range(16)])


def test_mix64_is_the_splitmix64_finaliser():
    # the first outputs of splitmix64 seeded with 0 (Vigna's splitmix64.c: state += G, then this finaliser)
    assert [int(v) for v in mr.mix64([mr.G, (2 * mr.G) & mr.MASK64])] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]
    assert int(mr.mix64(0)[0]) == 0


def test_draws_have_the_moments_of_independent_uniform_numbers(sample):
    r = sample
    n = r.size
    assert n == 196608
    assert r.min() >= -0.5 and r.max() < 0.5
    z_mean = r.mean() / np.sqrt(1.0 / 12.0 / n)                       # the mean of n uniforms has variance 1 / (12 n)
    z_var = (r.var() - 1.0 / 12.0) / np.sqrt(1.0 / 180.0 / n)         # their variance: (mu4 - sigma^4) / n = (1/80 - 1/144) / n

    def z_corr(a, b):                                                  # E[ab] = 0, Var[ab] = 1/144: the mean of m products
        return float((a * b).mean() * 12.0 * np.sqrt(a.size))

    z = {"mean": z_mean, "variance": z_var,
         "components 0-1": z_corr(r[..., 0], r[..., 1]), "components 1-2": z_corr(r[..., 1], r[..., 2]),
         "components 0-2": z_corr(r[..., 0], r[..., 2]),
         "consecutive steps": z_corr(r[:-1], r[1:]), "consecutive tags": z_corr(r[:, :-1], r[:, 1:])}
    print("  standard deviations from independence: " + ", ".join(f"{k} {v:+.2f}" for k, v in z.items()))
    for k, v in z.items():
        assert abs(v) <= 5.0, (k, v)


def test_a_draw_depends_on_seed_step_and_tag_only(sample):
    tags = np.arange(4096)
    perm = np.random.default_rng(0).permutation(4096)
    assert np.array_equal(mr.draws(12345, 7, tags[perm]), sample[7][perm])
    assert np.array_equal(mr.draws(12345, 7, [4095]), sample[7][4095:])
    assert np.array_equal(mr.draws(12345, 7, tags[100:200]), sample[7][100:200])
    # tags beyond 2^32 and negative ones (two's complement, as the kernel's cast) are atoms of their own
    big = mr.draws(12345, 7, np.array([5, 5 + (1 << 32), 5 + (1 << 33), -5], dtype=np.int64))
    assert len({row.tobytes() for row in big}) == 4 and np.array_equal(big[0], sample[7][5])


def test_seed_and_step_at_the_ends_of_the_range_neither_raise_nor_collide():
    tags = np.arange(64)
    seen = {}
    for seed in EDGE_WORDS + (12345,):
        for step in EDGE_WORDS + (12345,):
            r = mr.draws(seed, step, tags)
            assert r.shape == (64, 3) and r.min() >= -0.5 and r.max() < 0.5
            seen[(seed, step)] = r.tobytes()
    # no two seeds collide at one step, no two steps under one seed
    for fixed in EDGE_WORDS + (12345,):
        assert len({seen[(s, fixed)] for s in EDGE_WORDS}) == 3 and len({seen[(fixed, s)] for s in EDGE_WORDS}) == 3
    # The stream's key is the ONE word seed + G (step + 1): pairs with the same word are the same stream by construction, such as
    # (2^63, 2^63) and (0, 0), or seed + G at step t and seed at step t + 1.  As many streams as distinct words:
    assert len(set(seen.values())) == len({(s + mr.G * (t + 1)) & mr.MASK64 for s, t in seen}) < len(seen)
    assert seen[(1 << 63, 1 << 63)] == seen[(0, 0)] and seen[(0, 1 << 63)] == seen[(1 << 63, 0)]
    # the words are taken modulo 2^64, like the kernel's unsigned arguments
    assert mr.draws((1 << 64) + 3, 2, tags).tobytes() == mr.draws(3, 2, tags).tobytes()


def _langevin_factors(masses_of_atoms, T, damp, dt):
    """dtfm, g1, g2 exactly as VerletRun._per_atom_factors computes them: that method, on a stand-in for the run"""
    import torch
    from lammps_ani_amd import md
    species = torch.arange(len(masses_of_atoms), dtype=torch.int32)
    run = SimpleNamespace(nlocal=len(masses_of_atoms), dc=SimpleNamespace(multi=False), species=species,
                          masses=torch.as_tensor(np.asarray(masses_of_atoms, dtype=np.float64)), dt=dt, langevin=(T, damp))
    md.VerletRun._per_atom_factors(run)
    return run._dtfm1.numpy(), run._g1.numpy(), run._g2.numpy()


def test_verlet_run_refuses_a_device_without_the_library_entry_points():
    """every step of the loop is a device entry point of libani_hip: a CPU device is refused before anything else is touched"""
    import torch
    from lammps_ani_amd import md
    with pytest.raises(ValueError, match="device entry points"):
        md.VerletRun(None, None, np.ones(3), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="device entry points"):
        md.VerletRun(None, None, None, "cpu")


def free_particle_masses(n):
    from lammps_ani_amd import md
    return np.asarray(md.ANI2X_MASSES)[np.array([0, 1, 3])][np.random.default_rng(5).integers(0, 3, n)]      # H, C, O


def test_free_particles_under_the_thermostat_settle_at_the_exact_stationary_temperature():
    """Free particles (no force but the thermostat's) through final_initial_integrate: per step f = g1 v + g2 r, v += 2 s f, that is
    v <- (1 - a) v + 2 s g2 r with a = dt / damp (2 s g1 = -a), and (2 s g2)^2 / 12 = 2 a kT / (m mvv2e) is the variance of the
    kick.  Stationary: <v^2> = (1 - a)^2 <v^2> + 2 a kT / (m mvv2e), so m mvv2e <v^2> = kT / (1 - a / 2): the loop's discrete
    thermostat settles at T / (1 - dt / (2 damp)) exactly, 315.79 K for T = 300, damp = 10, dt = 1.

    Bar: the estimate is a mean of m mvv2e v^2 / k over 3 n components and 200 steps.  v^2 of one component decorrelates over
    damp / (2 dt) steps; counting one independent sample per 2 damp / dt = 20 steps (conservative) leaves
    N = 3 n 200 / 20 = 122 880 samples.  The variance of a sample of v^2 about <v^2> is 2 <v^2>^2 for a Gaussian v (v is a
    geometric sum of uniform kicks: its excess kurtosis, -1.2 (1 - q) / (1 + q) = -0.13 with q = (1 - a)^2, only lowers
    that), so the relative standard deviation of the estimate is sqrt(2 / N) = 0.40 %, and 5 of them 2.02 %.  Measured with
    these masses and seed 12345: 317.31 K, +0.48 %."""
    from lammps_ani_amd import md
    n, T, damp, dt, discard, keep = 4096, 300.0, 10.0, 1.0, 60, 200
    m = free_particle_masses(n)
    dtfm, g1, g2 = _langevin_factors(m, T, damp, dt)
    a = dt / damp
    assert np.allclose(2.0 * dtfm * g1, -a, rtol=1e-14, atol=0)
    assert np.allclose((2.0 * dtfm * g2) ** 2 / 12.0, 2.0 * a * md.BOLTZ * T / (m * md.MVV2E), rtol=1e-13, atol=0)
    x, v = np.zeros((n, 3)), np.zeros((n, 3))
    temps = []
    for step in range(discard + keep):
        x, v, _, _ = mr.final_initial_integrate(x, v, np.zeros((n, 3)), dtfm, dt, x, 0.0, 1, g1, g2, None, 12345, step)
        temps.append(float((m[:, None] * v * v).mean() * md.MVV2E / md.BOLTZ))
    got, want = float(np.mean(temps[discard:])), T / (1.0 - dt / (2.0 * damp))
    nsamples = 3 * n * keep / (2.0 * damp / dt)
    bar = 5.0 * np.sqrt(2.0 / nsamples)
    print(f"  stationary temperature {got:.2f} K against {want:.2f} K: {100 * (got / want - 1):+.2f} % (bar {100 * bar:.2f} %)")
    assert abs(got / want - 1.0) <= bar


def test_integrators_compose_and_fold_the_displacement_maximum():
    rng = np.random.default_rng(2)
    n = 300
    x, v, f = rng.uniform(0, 20, (n, 3)), rng.normal(0, 0.01, (n, 3)), rng.normal(0, 15, (n, 3))
    s, g1, g2 = rng.uniform(1e-4, 5e-4, n), -rng.uniform(100, 4000, n), rng.uniform(100, 4000, n)
    xb = x + rng.normal(0, 0.1, (n, 3))
    x1, v1, d1 = mr.initial_integrate(x, v, f, s, 0.5, xb, 0.0)
    assert np.array_equal(v1, v + s[:, None] * f) and np.array_equal(x1, x + 0.5 * v1)
    assert d1 == ((x1 - xb) ** 2).sum(1).max() or abs(d1 - ((x1 - xb) ** 2).sum(1).max()) < 1e-15
    assert mr.initial_integrate(x, v, f, s, 0.5, xb, 1e9)[2] == 1e9
    vf, ff = mr.final_integrate(v, f, s, 1, g1, g2, None, 3, 4)
    assert np.array_equal(ff, f + (g1[:, None] * v + g2[:, None] * mr.draws(3, 4, np.arange(n))))
    xa, va, fa, da = mr.final_initial_integrate(x, v, f, s, 0.5, xb, 0.0, 1, g1, g2, None, 3, 4)
    xe, ve, de = mr.initial_integrate(x, vf, ff, s, 0.5, xb, 0.0)
    assert np.array_equal(xa, xe) and np.array_equal(va, ve) and np.array_equal(fa, ff) and da == de
    assert np.array_equal(mr.final_integrate(v, f, s)[1], f)
    z = np.zeros((0, 3))
    assert mr.initial_integrate(z, z, z, np.zeros(0), 0.5, z, 3.5)[2] == 3.5


def test_ghost_operations_are_what_a_loop_over_the_ghosts_does():
    rng = np.random.default_rng(3)
    nl, ng = 7, 40
    owner = rng.integers(0, nl, ng)
    shift = rng.integers(-2, 3, (ng, 3)) * 10.0
    x = rng.uniform(0, 10, (nl + ng + 2, 3))
    f = rng.integers(-1000, 1000, (nl + ng + 2, 3)) / 8.0
    xf, fr_, fo = x.copy(), f.copy(), f.copy()
    ghost_of = rng.permutation(ng)
    for g in range(ng):
        xf[nl + g] = x[owner[g]] + shift[g]
        fr_[owner[g]] += f[nl + g]
        fo[owner[g]] += f[nl + ghost_of[g]]
    assert np.array_equal(mr.forward(x, owner, shift, nl), xf)
    assert np.array_equal(mr.pack(x, owner, shift), xf[nl:nl + ng])
    assert np.array_equal(mr.reverse(f, owner, nl), fr_)
    assert np.array_equal(mr.reverse_ordered(f, owner, None, nl), fr_)
    assert np.array_equal(mr.reverse_ordered(f, owner, ghost_of, nl), fo)
    assert np.array_equal(mr.unpack_reverse(f, owner, f[nl:nl + ng]), fr_)
    idx = rng.permutation(nl + ng + 2)[:11]
    assert np.array_equal(mr.gather(x, idx), np.stack([x[i] for i in idx]))
    sc = mr.scatter(x, idx, f[:11])
    assert np.array_equal(sc[idx], f[:11]) and np.array_equal(np.delete(sc, idx, 0), np.delete(x, idx, 0))
    sp = rng.integers(0, 7, nl + ng + 2).astype(np.int32)
    xa, spa = mr.append(x, sp, nl, owner, shift)
    assert np.array_equal(xa, xf) and np.array_equal(spa[nl:nl + ng], sp[owner]) and np.array_equal(spa[nl + ng:], sp[nl + ng:])
    assert np.array_equal(mr.forward(x, owner[:0], shift[:0], nl), x)


def test_wrap_exact_on_hand_worked_cases():
    F = Fraction
    assert mr.wrap_exact(0.25, 0.0, 1.0) == F(1, 4)
    assert mr.wrap_exact(-0.25, 0.0, 1.0) == F(3, 4)
    assert mr.wrap_exact(7.5, -2.0, 4.0) == F(-1, 2)                       # 7.5 - 2 * 4
    assert mr.wrap_exact(-2.0, -2.0, 4.0) == F(-2)                         # the lower face stays
    assert mr.wrap_exact(2.0, -2.0, 4.0) == F(-2)                          # the upper face is the lower one
    assert mr.wrap_exact(-6.0, -2.0, 4.0) == F(-2) and mr.wrap_exact(6.0, -2.0, 4.0) == F(-2)
    assert mr.wrap_exact(-10.5, 1.0, 3.0) == F(3, 2)                       # -10.5 + 4 * 3
    # one ulp below the lower face: the exact image is one (input) ulp below the upper face, not a double near it
    below = np.nextafter(1.0, 0.0)
    assert mr.wrap_exact(below, 1.0, 3.0) == F(4) - (F(1) - F(float(below))) and F(4) - mr.wrap_exact(below, 1.0, 3.0) == F(1, 2 ** 53)
    # decimal bounds are the doubles they round to: as doubles 0.1 + 0.2 > 0.3 in exact arithmetic, so 0.3 is inside
    # [0.1, 0.1 + 0.2) and 0.1 is ONE length below [0.3, 0.3 + 0.2)
    assert mr.wrap_exact(0.3, 0.1, 0.2) == F(0.3) and mr.wrap_exact(0.1, 0.3, 0.2) == F(0.1) + F(0.2)


COUNTER_EXAMPLES = ((4.4, 56.4, float.fromhex("-0x1.ap+5")), (36.3, 34.8, float.fromhex("-0x1.0a66666666667p+5")))


def test_the_plain_wrap_formula_leaves_the_box_below_the_lower_face():
    """The record of why wrap_kernel and DomainComm.exchange clamp at the lower face: in plain double precision
    v - floor((v - lo) / L) L returns values BELOW lo for inputs within a few ulp of lo + k L: the quotient rounds up to the
    integer, and the exact image, a hair under the upper face, comes out a hair under the lower one."""
    for lo, L, v in COUNTER_EXAMPLES:
        out = float(mr.wrap_plain(v, lo, L))
        t = mr.wrap_exact(v, lo, L)
        print(f"  lo {lo} L {L} v {v!r}: plain formula {out!r} = lo - {lo - out:.2e}; exact image lo + L - {float(Fraction(lo) + Fraction(L) - t):.2e}")
        assert out < lo and lo - out < 1e-14                              # NOT in [lo, lo + L)
        assert Fraction(lo) + Fraction(L) - t < Fraction(1, 10 ** 13)     # the exact image sits under the upper face
        assert float(mr.wrap_fixed(v, lo, L)) == lo
    # and it is no rarity: most boxes have such an input among the ulp-neighbours of lo + k L
    rng = np.random.default_rng(0)
    boxes = 0
    for _ in range(200):
        lo, L = round(rng.uniform(-50, 50), 1), round(rng.uniform(5, 80), 1)
        v = np.array([lo + k * L for k in (-1, 1, 2)])
        v = np.concatenate([v] + [np.nextafter(v, s * np.inf) for s in (-1, 1)])
        out, fixed = mr.wrap_plain(v, lo, L), mr.wrap_fixed(v, lo, L)
        boxes += bool((out < lo).any())
        assert (fixed >= lo).all() and (fixed < lo + L).all()
    assert boxes > 20, boxes


@pytest.mark.parametrize("periodic", [(True, True, True), (True, False, True)], ids=["periodic", "slab"])
def test_the_tensor_form_of_the_wrap_is_the_clamped_formula(periodic):
    """comm.DomainComm.exchange on one rank (both of its branches) is wrap_fixed bit for bit -- torch on the CPU fuses nothing --
    and stays in [lo, lo + L) on the counter-examples and the ulp-neighbours of the faces' images"""
    import torch
    from lammps_ani_amd import comm
    lo, L = np.array([4.4, 36.3, -12.7]), np.array([56.4, 34.8, 25.1])
    cols = []
    for k in range(3):
        v = np.array([lo[k] + j * L[k] for j in (-1, 0, 1, 2)])
        v = np.concatenate([v] + [np.nextafter(v, s * np.inf) for s in (-1, 1)] + [[c[2] for c in COUNTER_EXAMPLES if c[0] == lo[k]]])
        cols.append(np.resize(v, 16))
    x = np.stack(cols, axis=1)
    dc = comm.DomainComm((1, 1, 1), lo, L, 7.1, "cpu", periodic=periodic)
    out = dc.exchange(torch.as_tensor(x))[0].numpy()
    for k in range(3):
        if periodic[k]:
            assert out[:, k].tobytes() == mr.wrap_fixed(x[:, k], lo[k], L[k]).tobytes()
            assert (out[:, k] >= lo[k]).all() and (out[:, k] < lo[k] + L[k]).all()
        else:
            assert out[:, k].tobytes() == x[:, k].tobytes()
    assert (mr.wrap_plain(x[:, 0], lo[0], L[0]) < lo[0]).any()              # the inputs do include the failing kind


def _shell_brute(x, clo, chi, cshift):
    n, ncombo = len(x), len(clo)
    nblk = max((n + 255) // 256, 1)
    cnt = [0] * (ncombo * nblk)
    idx, shift, per = [], [], [0] * ncombo
    for c in range(ncombo):
        for a in range(n):
            if all(clo[c][k] <= x[a][k] < chi[c][k] for k in range(3)):
                cnt[c * nblk + a // 256] += 1
                per[c] += 1
                idx.append(a)
                shift.append(list(cshift[c]))
    off = [sum(cnt[:i]) for i in range(len(cnt))]
    return cnt, off, [len(idx)] + per, idx, shift


@pytest.mark.parametrize("n,ncombo", [(0, 3), (1, 1), (5, 4), (40, 7), (300, 5)])
def test_shell_against_a_loop(n, ncombo):
    rng = np.random.default_rng(10 * n + ncombo)
    x = rng.integers(0, 8, (n, 3)) * 0.5                                   # a coarse grid: atoms land ON the faces
    clo = rng.integers(0, 5, (ncombo, 3)) * 0.5
    chi = clo + rng.integers(1, 6, (ncombo, 3)) * 0.5
    cshift = rng.integers(-1, 2, (ncombo, 3)) * 4.0
    cnt, off, counts, idx, shift, ghosts = mr.shell(x, clo, chi, cshift)
    bc, bo, bcounts, bidx, bshift = _shell_brute(x.tolist(), clo.tolist(), chi.tolist(), cshift.tolist())
    assert cnt.tolist() == bc and off.tolist() == bo and counts.tolist() == bcounts and idx.tolist() == bidx
    assert shift.tolist() == bshift and shift.shape == (len(bidx), 3)
    assert np.array_equal(ghosts, x[bidx] + np.asarray(bshift).reshape(-1, 3))
    if n >= 40:
        on_lo = ((x[None] == clo[:, None]).any(-1) & ((x[None] >= clo[:, None]) & (x[None] < chi[:, None])).all(-1)).any()
        assert on_lo and (x[None] == chi[:, None]).any()                   # the faces are exercised


def test_shell_faces_one_atom():
    one = np.array([[1.0, 2.0, 3.0]])
    for clo, chi, hit in (([1, 2, 3], [2, 3, 4], 1), ([0, 1, 2], [1, 3, 4], 0), ([0, 1, 2], [2, 3, 3], 0), ([1, 2, 3], [1, 3, 4], 0),
                          (np.nextafter([1.0, 2.0, 3.0], 9.0), [2, 3, 4], 0), ([0, 0, 0], np.nextafter([1.0, 2.0, 3.0], 9.0), 1)):
        out = mr.shell(one, [clo], [chi], [[5.0, 0.0, -5.0]])
        assert out[2].tolist() == [hit, hit] and out[0].tolist() == [hit] and out[1].tolist() == [0]
        if hit:
            assert out[5].tolist() == [[6.0, 2.0, -2.0]]


def test_check():
    assert mr.check(2.5, -100.0) == (2.5, 0.0)
    for e in (float("nan"), float("inf"), -float("inf")):
        assert mr.check(2.5, e) == (float("inf"), 0.0)
