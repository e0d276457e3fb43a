"""AEV stream tables (option aev_stream_tables, include/ani_hip.h): which pair of a centre's angular neighbours a lane of the fast AEV
kernels takes in a step depends on the centre's per-species neighbour counts alone; the kernels read it as one word per lane and
step from tables kept per tuple of counts instead of decoding it arithmetically.

  * table contents: the two stream orders restated in numpy, word for word and length for length;
  * option 1 against option 0 on the same handle and input: AEV rows bitwise, forces / energy / virial to the order of the atomic
    sums (the bars of test_hip_properties.py for aev_symmetric_radial 1 against 0);
  * the tables are built when the set of species present is installed, not per neighbour list, and not at all for three or more
    species."""
import numpy as np
import pytest

from lammps_ani_amd import harness as hx
from oracle import Oracle

F_TOL = 2.3e-3     # kcal/mol/A, as tests/test_hip_properties.py
NT = 32            # bound on either count of a two-species layout
K_MAX_ANG = 96     # angular capacity: bound of a one-species layout
RCA = 3.5          # angular cutoff of the synthetic ANI-1x / ANI-2x models
NA, NZ = 8, 4      # ANI-2x angular grid: 64 / NA = 8 slots pad a forward bucket


@pytest.fixture(scope="module")
def hip():
    from lammps_ani_amd import ani_hip
    return ani_hip


# ---- the two stream orders, restated ------------------------------------------------------------------------------------------
def _buckets(counts):
    """(bucket index among all S (S + 1) / 2 species pairs, s1, s2) in the kernels' order: s1 <= s2, row-major"""
    S = len(counts)
    return [(b, s1, s2) for b, (s1, s2) in enumerate((s1, s2) for s1 in range(S) for s2 in range(s1, S))]


def backward_stream(counts):
    """Words of the backward stream of a centre with counts[s] angular neighbours of species s (the comment above
    build_pair_table): per non-empty bucket, bands of two adjacent ROW neighbours walk the bucket's column slots together, the lower
    half-wave on the even row, the upper on the odd one.  A triangular bucket (pairs a < b of n neighbours): bands k < n / 2 of rows
    2k, 2k + 1 with n - 1 - 2k slots, column 2k + 1 + slot, the odd row idle at slot 0 -- floor(n^2 / 4) slots.  A rectangular one:
    the smaller group is the rows (the first on a tie), ceil(rows / 2) bands of one slot per column, an odd last row idle."""
    start = np.concatenate([[0], np.cumsum(counts)])
    words, nbk = [], 0
    for b, s1, s2 in _buckets(counts):
        n1, n2 = counts[s1], counts[s2]
        before = len(words)
        if s1 == s2:
            for k in range(n1 // 2):
                for c in range(n1 - 1 - 2 * k):
                    ia, ib = start[s1] + 2 * k, start[s1] + 2 * k + 1 + c
                    words.append(ia | ib << 8 | c << 16 | b << 24 | 1 << 29 | 1 << 30 | (1 if c >= 1 else 0) << 31)
        elif n1 > 0 and n2 > 0:
            rows, cols = (s2, s1) if n2 < n1 else (s1, s2)
            nr, nc = counts[rows], counts[cols]
            for k in range((nr + 1) // 2):
                for c in range(nc):
                    ia, ib = start[rows] + 2 * k, start[cols] + c
                    words.append(ia | ib << 8 | c << 16 | b << 24 | 0 << 29 | 1 << 30 | (1 if 2 * k + 1 < nr else 0) << 31)
        nbk += len(words) > before
    return np.array(words, dtype=np.int64).astype(np.uint32), nbk


def forward_stream(counts, q=64 // NA):
    """Words of the forward stream (build_bucket_table, stream_pair): per non-empty bucket its pairs -- triangular: a < b row-major
    over the strict upper triangle; rectangular: a over the first species, b over the second, b fastest -- padded to a multiple of
    q slots with invalid words that point at the first neighbour of either group (a triangular bucket: at its first two)."""
    start = np.concatenate([[0], np.cumsum(counts)])
    words, nbk = [], 0
    for b, s1, s2 in _buckets(counts):
        n1, n2 = counts[s1], counts[s2]
        pairs = [(a, c) for a in range(n1) for c in range(a + 1, n1)] if s1 == s2 else [(a, c) for a in range(n1) for c in range(n2)]
        if not pairs:
            continue
        nbk += 1
        for a, c in pairs:
            words.append((start[s1] + a) | (start[s2] + c) << 8 | b << 16 | 1 << 24)
        for _ in range(-len(pairs) % q):
            words.append(start[s1] | (start[s2] + (1 if s1 == s2 else 0)) << 8 | b << 16 | 0 << 24)
    return np.array(words, dtype=np.int64).astype(np.uint32), nbk


def _angular_counts(inp, S):
    """[nlocal][S] neighbours of each species inside Rca, from the positions (fp64; no pair of the boxes below sits within 1e-6 of Rca)"""
    i = np.repeat(np.arange(inp.nlocal), inp.numneigh)
    d = np.linalg.norm(inp.x[inp.jlist] - inp.x[i], axis=1)
    assert np.abs(d - RCA).min() > 1e-6
    sp = np.searchsorted(np.unique(inp.species), inp.species)[inp.jlist]   # compact species, as the library's map
    out = np.zeros((inp.nlocal, S), int)
    np.add.at(out, (i[d <= RCA], sp[d <= RCA]), 1)
    return out


def _dense_two_species_box():
    """(b): 420 atoms of two species in an 11.1 A box (0.31 per A^3): a centre has ~28 +- 5 neighbours of either species inside Rca.
    A list skin of 0.3 A keeps the candidate lists inside the fused forward kernel's 256."""
    return hx.decompose(hx.random_box(420, 2, 11.1, seed=1), cutoff=5.1, skin=0.3)


def _clusters():
    """(d): far apart in an open box -- an isolated O; an O-H pair (one neighbour: no angular pair); H-O-H (one pair); an O with four
    H inside Rca (every neighbour of one species; the H see both species)."""
    x = [[0, 0, 0], [20, 0, 0], [20.96, 0, 0], [40, 0, 0], [40.96, 0, 0], [39.76, 0.93, 0],
         [60, 0, 0], [60.96, 0, 0], [59.04, 0, 0], [60, 0.96, 0], [60, -0.96, 0.1]]
    t = [4, 4, 1, 4, 1, 1, 4, 1, 1, 1, 1]
    sysm = hx.System(np.array(x, float), np.array(t, np.int32), np.full(3, -15.0), np.full(3, 75.0), (False, False, False))
    return hx.decompose(sysm)


def _real_rows(ani, nlocal):
    v = ani.debug_view()
    rows = ani.debug_read(v.d_row_of_centre, (nlocal,), np.int32)
    return ani.debug_read(v.d_aev, (v.nrows, v.aev_stride), np.float32)[rows]


# ---- 1. table contents --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_table_contents_equal_the_restated_stream_orders(model_cache, hip):
    p = model_cache("ani2x", 1, 2024)
    lens_b, lens_f = [], []
    cases = [(hx.decompose(hx.random_box(60, 1, 14.0, seed=4)), [(n,) for n in (0, 1, 2, 3, 31, 32, 33, K_MAX_ANG)]),
             (hx.decompose(hx.water_box(96, seed=3)), [(a, b) for a in range(13) for b in range(13)] +
              [(NT, NT), (NT, 0), (0, NT), (NT, 1), (1, NT)])]
    for inp, tuples in cases:
        ani = hip.ANI(p, 0)
        ani.compute(inp, ago=0)
        t = ani.stream_tables()
        S = len(tuples[0])
        assert t["species"] == S and t["bound"] == (K_MAX_ANG if S == 1 else NT)
        assert t["tuples"] == (t["bound"] + 1) ** S
        for counts in tuples:
            ix = counts[0] if S == 1 else counts[0] * (t["bound"] + 1) + counts[1]
            for key, ref, step, lens in (("bwd", backward_stream, 32, lens_b), ("fwd", forward_stream, 64, lens_f)):
                want, nbk = ref(list(counts))
                off, length, buckets, reserved = (int(v) for v in t["desc_" + key][ix])
                assert (length, buckets, reserved) == (len(want), nbk, -(-len(want) // step) * step), (key, counts)
                assert off + reserved <= len(t["words_" + key])
                assert np.array_equal(t["words_" + key][off: off + length], want), (key, counts)
                lens.append(length)
        ani.close()
    # The tuples compared meet every step boundary of the streams from both sides.  The block of all (n0, n1) <= 12 is what makes
    # this possible (its lengths are dense; the few large tuples beside it are single points), so the multiples it passes are the
    # ones asked about.  "Just below" a multiple m: the last step more than half full (m - step / 2 <= length < m); "just above":
    # one more step, less than half full (m < length <= m + step / 2).
    dense_b = max(len(backward_stream([a, b])[0]) for a in range(13) for b in range(13))
    dense_f = max(len(forward_stream([a, b])[0]) for a in range(13) for b in range(13))
    for lens, step, top in ((lens_b, 32, dense_b), (lens_f, 64, dense_f)):
        for m in range(step, top, step):
            assert any(m - step // 2 <= v < m for v in lens) and any(m < v <= m + step // 2 for v in lens), (step, m)


# ---- 2. option 1 against option 0 ---------------------------------------------------------------------------------------------
def _on_off(ani, inp, vflag=True, fused=1):
    out = []
    ani.set_option("aev_fused", fused)
    for on in (1, 0):
        ani.set_option("aev_stream_tables", on)
        r = ani.compute(inp, ago=0, eflag_atom=True, vflag=vflag)
        r["aev"] = _real_rows(ani, inp.nlocal)
        out.append(r)
    ani.set_option("aev_stream_tables", 1)
    ani.set_option("aev_fused", 1)
    return out


def _assert_same(on, off, inp, vflag=True):
    assert np.array_equal(on["aev"].view(np.uint32), off["aev"].view(np.uint32))   # the forward kernels sum in a fixed order
    fmax = max(1.0, float(np.abs(off["force"]).max()))
    assert np.abs(on["force"] - off["force"]).max() < 0.02 * F_TOL * fmax
    assert abs(on["energy"] - off["energy"]) < 1e-5
    if vflag:
        assert np.abs(on["virial"] - off["virial"]).max() < 2e-3 * max(1.0, inp.nlocal / 100.0)


@pytest.mark.gpu
def test_tables_equal_the_arithmetic_decode_on_water(model_cache, hip):
    """(a) water with its periodic ghosts: both forward kernels, the backward kernel with and without the virial (the benchmark runs
    without); forces against the oracle."""
    p = model_cache("ani2x", 2, 79)
    inp = hx.decompose(hx.water_box(3000, seed=3))
    ref = Oracle(p).compute(inp)
    ani = hip.ANI(p, 0)
    for vflag, fused in ((True, 1), (False, 1), (True, 0)):
        on, off = _on_off(ani, inp, vflag=vflag, fused=fused)
        assert ani.stream_tables(contents=False)["species"] == 2
        _assert_same(on, off, inp, vflag=vflag)
        assert np.abs(on["force"] - ref["force"]).max() < F_TOL
        assert np.abs(off["force"] - ref["force"]).max() < F_TOL
    ani.close()


@pytest.mark.gpu
def test_centres_above_the_bound_fall_back_in_the_same_launch(model_cache, hip):
    """(b) a dense two-species box: some centres have more than NT neighbours of one species inside Rca and decode arithmetically,
    the others read the tables, in one launch."""
    inp = _dense_two_species_box()
    c = _angular_counts(inp, 2)
    above = (c > NT).any(1)
    assert above.sum() >= 20 and (~above).sum() >= 20 and c.sum(1).max() <= K_MAX_ANG and inp.numneigh.max() <= 256
    p = model_cache("ani2x", 2, 79)
    ref = Oracle(p).compute(inp)
    ani = hip.ANI(p, 0)
    for fused in (1, 0):
        on, off = _on_off(ani, inp, fused=fused)
        assert ani.debug_view().error_flags == 0
        _assert_same(on, off, inp)
        print("dense box: max |F - oracle|", np.abs(on["force"] - ref["force"]).max(), np.abs(off["force"] - ref["force"]).max(),
              "max |F|", np.abs(ref["force"]).max())
        assert np.abs(on["force"] - ref["force"]).max() < F_TOL
        assert np.abs(off["force"] - ref["force"]).max() < F_TOL
    ani.close()


@pytest.mark.gpu
def test_one_species_clusters_and_seven_species(model_cache, hip):
    """(c) one species (counts up to the angular capacity are tabled), (d) tiny clusters: no neighbour, no pair, one pair, all
    neighbours of one species, (e) seven species: no tables, the option changes nothing."""
    p = model_cache("ani2x", 2, 79)
    one = hx.decompose(hx.random_box(300, 1, 12.5, seed=4))
    c = _angular_counts(one, 1)
    assert c.max() > NT and c.max() <= K_MAX_ANG
    clusters = _clusters()
    assert sorted(_angular_counts(clusters, 2).sum(1).tolist()) == [0, 1, 1, 2, 2, 2, 4, 4, 4, 4, 4]
    for inp, species in ((one, 1), (clusters, 2), (hx.decompose(hx.random_box(1200, 7, 26.0, seed=6)), 0)):
        ani = hip.ANI(p, 0)
        for fused in (1, 0):
            on, off = _on_off(ani, inp, fused=fused)
            assert ani.stream_tables(contents=False)["species"] == species
            _assert_same(on, off, inp)
        ani.close()


# ---- 3. set-up behaviour ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tables_are_built_per_species_map_not_per_list(model_cache, hip):
    p = model_cache("ani2x", 1, 2024)
    ani = hip.ANI(p, 0)
    assert ani.stream_tables(contents=False)["builds"] == 0
    water = hx.decompose(hx.water_box(300, seed=2))
    ani.compute(water, ago=0)
    a = ani.stream_tables(contents=False)
    assert a["species"] == 2 and a["builds"] == 1 and a["words_bwd"] > 0 and a["words_fwd"] > 0
    assert 4 * (a["words_bwd"] + a["words_fwd"]) + 32 * a["tuples"] <= 8 << 20   # the cap on a handle's tables
    ani.compute(hx.decompose(hx.water_box(600, seed=5)), ago=0)   # a re-neighbouring, another list: same species
    ani.compute(water, ago=0)
    b = ani.stream_tables(contents=False)
    assert b == a                                                 # same addresses, same sizes, not built again
    ani.compute(hx.decompose(hx.random_box(200, 3, 16.0, seed=1)), ago=0)
    c = ani.stream_tables(contents=False)
    assert c["species"] == 0 and c["tuples"] == 0 and c["words_bwd"] == 0 and c["d_words_bwd"] is None
    ani.close()


# ---- the restated orders against plain enumerations (no GPU) ------------------------------------------------------------------
def test_restated_streams_enumerate_every_pair_once():
    for counts in ([0], [1], [2], [5], [0, 0], [3, 0], [0, 4], [1, 1], [4, 7], [7, 4], [5, 5], [12, 12], [NT, NT]):
        start = np.concatenate([[0], np.cumsum(counts)])
        n = int(start[-1])
        want = sorted((a, b) for a in range(n) for b in range(a + 1, n))
        w, _ = forward_stream(counts)
        v = w[(w >> 24) & 1 == 1]
        assert sorted(zip((v & 0xff).tolist(), ((v >> 8) & 0xff).tolist())) == want and len(w) % (64 // NA) == 0
        w, _ = backward_stream(counts)
        got = []
        for h in (0, 1):
            v = w[(w >> (30 + h)) & 1 == 1]
            got += [tuple(sorted(t)) for t in zip(((v & 0xff) + h).tolist(), ((v >> 8) & 0xff).tolist())]
        assert sorted(got) == want
