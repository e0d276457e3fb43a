"""CPU: tests/repulsion_reference.py -- the numpy fp64 pair sum of the repulsion alone, its bars and its mutations -- against the
oracle on null models, for every case tests/test_repulsion_kernels.py runs on the device.

The oracle's ``eatom`` on a null model is exactly 0: the repulsion is not part of ``eatom``, neither in the oracle (pass C adds
it to the total only) nor in ``finish_kernel`` (``repulsion_energy_kernel`` adds it to ev[0] afterwards).
"""
import numpy as np
import pytest

import repulsion_reference as rr
from lammps_ani_amd import model_file as mf

INPUTS = [(c, (1, 1, 1), 0) for c in rr.CASES] + [("mixed64", (2, 1, 1), 0), ("mixed64", (2, 1, 1), 1)]
IDS = [c if g == (1, 1, 1) else f"{c}-brick{r}" for c, g, r in INPUTS]
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    """after the module: bars, caps, fp32-model errors and mutation ratios per case, on stdout (pytest -s shows it)"""
    yield
    for k in sorted(RATIOS):
        print(f"repulsion reference {k}: {RATIOS[k]}")


@pytest.fixture(scope="module")
def oracle_of(tmp_path_factory):
    from oracle import Oracle
    d = tmp_path_factory.mktemp("null_models")
    cache = {}

    def get(case):
        if case not in cache:
            p = str(d / f"{case}.anim")
            mf.write_model(p, rr.case_model(case))
            cache[case] = Oracle(p)
        return cache[case]

    return get


@pytest.mark.parametrize("case,grid,rank", INPUTS, ids=IDS)
def test_reference_equals_oracle_on_the_null_model(case, grid, rank, oracle_of):
    inp, m, ref, _, _ = rr.case_reference(case, grid, rank)
    o = oracle_of(case).compute(inp)
    assert np.all(o["eatom"] == 0.0)
    for q in ("force", "virial"):
        big = float(np.abs(ref[q]).max())
        assert np.abs(o[q] - ref[q]).max() <= 1e-10 * big, q
    assert abs(o["energy"] - ref["energy"]) <= 1e-10 * abs(ref["energy"])
    assert np.abs(ref["force"]).max() > 50.0     # the wall is in the case
    if case == "seven":
        t = ref["terms"]
        radial = np.bincount(t["i"], weights=(t["r"] <= m.Rcr).astype(np.float64), minlength=inp.nlocal)
        assert radial.max() > 64 and np.abs(ref["force"]).max() < 2000.0 and len(np.unique(inp.species)) == 7
    if case == "water-HO":
        assert list(np.unique(inp.species)) == [0, 3]
    if case == "soft-cut60":
        t = ref["terms"]
        assert np.any((t["r"] > m.Rcr) & (t["sh"] != 0)) and float(np.max(inp.numneigh)) > 0


@pytest.mark.parametrize("case,grid,rank", INPUTS, ids=IDS)
def test_bars_caps_and_the_fp32_arithmetic_model(case, grid, rank):
    """Each bar is at most its cap; the fp32 evaluation of the pair function (numpy, r rounded to float, the kernels' operations)
    stays inside the fp32 error model WITHOUT the margin, in every output; the fp64 bars are no looser than the existing ones."""
    inp, m, ref, b32, b64 = rr.case_reference(case, grid, rank)
    for b in (b32, b64):
        for q in ("force", "energy", "virial", "atom_virial"):
            assert np.all(np.asarray(b[q]) <= np.asarray(b["cap"][q]))
    # the absolute energy cap is reachable in fp32 at all: MARGIN roundings of the whole energy stay below it (see CASES)
    assert rr.MARGIN * rr.U32 * abs(ref["energy"]) <= b32["cap"]["energy"]
    assert b64["force"].max() <= rr.F_TOL64 and b64["energy"] <= rr.E_REL64 * abs(ref["energy"]) and b64["virial"] <= rr.V_TOL64
    r32 = rr.reference(inp, m.repulsion, real=np.float32)
    mdl = b32["model"]
    worst = dict(force=float(rr.ratio(np.abs(r32["force"] - ref["force"]).max(1), mdl["force"]).max()),
                 energy=abs(r32["energy"] - ref["energy"]) / mdl["energy"],
                 virial=float(np.abs(r32["virial"] - ref["virial"]).max()) / mdl["virial"],
                 atom_virial=float(rr.ratio(np.abs(r32["atom_virial"](9) - ref["atom_virial"](9)).max(1), mdl["atom_virial"]).max()))
    RATIOS[f"{case}/{grid}/{rank} fp32 numpy / model"] = {k: f"{v:.2f}" for k, v in worst.items()}
    RATIOS[f"{case}/{grid}/{rank} bars"] = (f"F max {b32['force'].max():.2e} (cap {b32['cap']['force']:.2e}) E {b32['energy']:.2e} (cap "
                                            f"{b32['cap']['energy']:.2e}) V {b32['virial']:.2e} (cap {b32['cap']['virial']:.2e}); fp64 F max "
                                            f"{b64['force'].max():.2e} E {b64['energy']:.2e} V {b64['virial']:.2e}")
    for q, v in worst.items():
        assert v <= 1.0, (q, v)


@pytest.mark.parametrize("case,grid,rank", INPUTS, ids=IDS)
def test_every_applicable_mutation_moves_the_reference_by_ten_bars(case, grid, rank):
    """What makes the device test able to fail: each single fault moves some atom's force, or the energy, by >= 10x the case's bar."""
    inp, m, ref, b32, b64 = rr.case_reference(case, grid, rank)
    r32 = rr.mutation_ratios(inp, m.repulsion, m.Rcr, ref, b32)
    r64 = rr.mutation_ratios(inp, m.repulsion, m.Rcr, ref, b64)
    RATIOS[f"{case}/{grid}/{rank} mutations / fp32 bar"] = {k: f"{v:.3g}" for k, v in r32.items()}
    assert {"no_dfc", "energy_whole"} <= set(r32)
    if case == "water-HO":
        assert "compact_tables" in r32
    if case == "soft-cut60":
        assert "beyond_rcr" in r32
    if inp.nghost:
        assert "ghost_whole" in r32
    for name in r32:
        assert r32[name] >= 10.0 and r64[name] >= 10.0, (name, r32[name], r64[name])


def test_forces_are_derivatives_of_the_energy_on_the_open_cluster():
    """Central differences of the reference energy, h = 2e-5 A: truncation h^2 |E''''| / 6 ~ 4e-10 / 6 * 1e5 < 1e-5 kcal/mol/A,
    rounding 1e-16 * 400 / h = 2e-9; bar 1e-6 of the largest force (1e-3 kcal/mol/A)."""
    import dataclasses
    inp, m, ref, _, _ = rr.case_reference("open40-ani1x")
    assert inp.nghost == 0
    h = 2e-5
    fd = np.zeros_like(ref["force"])
    for a in range(inp.ntotal):
        for k in range(3):
            e = []
            for sgn in (1.0, -1.0):
                x = inp.x.copy()
                x[a, k] += sgn * h
                e.append(rr.reference(dataclasses.replace(inp, x=x), m.repulsion)["energy"])
            fd[a, k] = -(e[0] - e[1]) / (2 * h)
    assert np.abs(fd - ref["force"]).max() <= 1e-6 * np.abs(ref["force"]).max()


def test_second_derivative_used_by_the_error_model():
    """e''/2 (the rounding-of-r term) against central differences of e'/2 in r"""
    inp, m, ref, _, _ = rr.case_reference("mixed64")
    t = ref["terms"]
    live = (t["sh"] != 0) & (t["r"] < 0.98 * t["cut"])
    r, h = t["r"][live], 1e-6
    y, al, k = t["y"][live], t["al"][live], t["k"][live]
    up = rr._pair_function(r + h, y, al, k, t["cut"], np.float64)[2]
    dn = rr._pair_function(r - h, y, al, k, t["cut"], np.float64)[2]
    d2 = rr.second_derivative(t)[live]
    assert np.all(np.abs((up - dn) / (2 * h) - d2) <= 1e-6 * np.abs(d2) + 1e-12)


def test_rank_energies_sum_to_the_one_rank_energy():
    one = rr.case_reference("mixed64")[2]["energy"]
    parts = [rr.case_reference("mixed64", (2, 1, 1), r)[2]["energy"] for r in (0, 1)]
    assert abs(sum(parts) - one) <= 1e-12 * abs(one)
    assert min(parts) > 0.1 * one


def test_null_model_and_file_roundtrip(tmp_path):
    m = rr.case_model("mixed64-cut51")
    assert m.repulsion["cutoff"] == 5.1 and m.Rcr == 5.2
    assert all(not W.any() and not b.any() for per_s in m.weights for per_l in per_s for W, b in per_l) and not m.self_energies.any()
    p = str(tmp_path / "n.anim")
    mf.write_model(p, m)
    back = mf.read_model(p)
    assert back.repulsion["cutoff"] == 5.1 and np.array_equal(back.repulsion["y_ab"], m.repulsion["y_ab"])
    assert rr.case_model("mixed64", repulsion=False).repulsion is None
