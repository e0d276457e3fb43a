"""GPU: VerletRun.minimize (device-resident FIRE, include/ani_md.h ani_md_fire_*) against the numpy FIRE of tests/fire_reference.py
with the CPU oracle as its calculator, iteration by iteration: etol = ftol = 0 and maxiter = K, so both sides make exactly K moves.

Cases (tests/fire_reference.py ORACLE_CASES, validated on the CPU by tests/test_fire_reference_cpu.py): the reference's 30-atom
water box with K = 25 and water_box(258) -- two blocks, the second holding two atoms -- with K = 12, each in both handle precisions.
Through check_every = 1 every iteration is recorded: dt, alpha, the counters (equal to the reference: the scalars and the branch
sequence), the energy, the forces and the positions modulo the box (the bars of tests/test_trajectory_vs_oracle.py: fp32
atol = rtol = 1e-3; fp64 atol 1e-9, rtol 1e-5, the energy as there).
"""
import numpy as np
import pytest

import fire_reference as fr
from lammps_ani_amd import harness as hx

pytestmark = pytest.mark.gpu

MODEL = ("ani2x", 8, 2024)
PRECISIONS = pytest.mark.parametrize("single", [True, False], ids=["precision_single", "precision_double"])


def _bars(single):
    return (1e-3, 1e-3) if single else (1e-9, 1e-5)


def _minimize(name, single, model_path, maxiter=None, check_every=1, skin=2.0, keep=False):
    """VerletRun.minimize on a case; returns (per-look records, result dict, final global x, extras)"""
    import torch
    from lammps_ani_amd import ani_hip, md
    sysm, p = fr.case_system(name), fr.case_params(name)
    inp = hx.decompose(sysm)
    ani = ani_hip.ANI(model_path, 0, -1, use_single=single)
    run = md.VerletRun(ani, inp, sysm.boxhi - sysm.boxlo, torch.device("cuda:0"), dt=0.1, every=7, skin=skin, box_lo=sysm.boxlo)
    n = sysm.natoms
    tag = run.tag.cpu().numpy()
    looks = []

    def glob(t):
        out = np.zeros((n, 3))
        out[tag] = t[:n].cpu().numpy()
        return out

    def on_look(rec):
        looks.append(dict(rec, x=glob(run.x), f=glob(run.f), builds=run.nbuilds))

    step_no = run.step_no
    fire = {k: p[k] for k in ("dtmax", "dtmin", "dtgrow", "dtshrink", "alpha0", "alphashrink", "delaystep", "initialdelay",
                              "halfstepback", "dmax")}
    res = run.minimize(0.0, 0.0, p["maxiter"] if maxiter is None else maxiter, dt0=p["dt0"], check_every=check_every,
                       on_look=on_look, **fire)
    assert run.step_no == step_no and float(run.v.abs().max()) == 0.0
    x = glob(run.x)
    if keep:
        return looks, res, x, (run, ani, glob)
    ani.close()
    return looks, res, x, None


def _follow(name, single, looks, res, hist, L, notes):
    atol, rtol = _bars(single)
    K = len(hist) - 1
    assert len(looks) == K + 1
    worst = dict(f=0.0, x=0.0, e=0.0)
    for k, (g, r) in enumerate(zip(looks, hist), start=1):
        # the scalars and the branch sequence: equal
        for key in ("iterations", "dt", "alpha", "last_negative", "uphill", "limited", "stop"):
            assert g[key] == r[key], (k, key, g[key], r[key])
        dx = g["x"] - r["x"]
        dx -= L * np.round(dx / L)                       # the loop wraps owned atoms into the box at a re-neighbouring
        worst["f"] = max(worst["f"], np.abs(g["f"] - r["f"]).max())
        worst["x"] = max(worst["x"], np.abs(dx).max())
        worst["e"] = max(worst["e"], abs(g["e_cur"] - r["E"]))
        assert np.allclose(g["f"], r["f"], rtol, atol), (k, np.abs(g["f"] - r["f"]).max())
        assert np.allclose(dx, 0.0, rtol, max(atol, 1e-12)), (k, np.abs(dx).max())
        pe_atol = atol if single else 1e-9 * max(1.0, abs(r["E"]) * 1e-3)
        assert np.allclose(g["e_cur"], r["E"], rtol, pe_atol), (k, g["e_cur"], r["E"])
        # |dP| <= |dv| |f| + |v| |df| (Cauchy-Schwarz): a few force bars of sqrt(vv ff); the sign is the branch
        assert abs(g["P"] - r["P"]) <= atol + 10 * rtol * np.sqrt(r["vv"] * r["ff"]) and (g["P"] > 0) == (r["P"] > 0)
    line = (f"{name} {'fp32' if single else 'fp64'}: {K} iterations, uphill {int(looks[-1]['uphill'])}, limited {int(looks[-1]['limited'])}, "
            f"rebuilds {res['rebuilds']}; max |dF| {worst['f']:.2e} kcal/mol/A, |dx| {worst['x']:.2e} A, |dE| {worst['e']:.2e} kcal/mol")
    print(line)
    notes.append(line)
    assert res["iterations"] == K and res["stop"] == "maxiter" and res["force_evaluations"] == K + 1
    assert res["uphill_events"] == hist[-1]["uphill"] and res["limited_moves"] == hist[-1]["limited"]
    # the energy after is below the energy before, and so is the force norm; both are the reference's
    assert res["energy_after"] < res["energy_before"] and res["fnorm_after"] < res["fnorm_before"]
    assert np.isclose(res["energy_before"], hist[0]["E"], rtol, 1e-3) and np.isclose(res["energy_after"], hist[-1]["E"], rtol, 1e-3)
    assert np.isclose(res["fnorm_before"], np.sqrt(hist[0]["ff"]), rtol, atol) and \
        np.isclose(res["fnorm_after"], np.sqrt(hist[-1]["ff"]), 10 * rtol, 10 * atol)


@pytest.fixture(scope="module")
def notes():
    lines = []
    yield lines
    print("\n".join(["FIRE minimisation against the oracle-driven reference, largest deviations:"] + lines))


@PRECISIONS
@pytest.mark.parametrize("name", ["water30", "water258"])
def test_minimize_follows_the_oracle_driven_reference(name, single, model_cache, notes):
    path = model_cache(*MODEL)
    sysm, p, hist = fr.oracle_case_run(name, path)
    looks, res, _, _ = _minimize(name, single, path)
    _follow(name, single, looks, res, hist, sysm.boxhi - sysm.boxlo, notes)


@PRECISIONS
def test_a_reneighbouring_inside_the_minimisation_still_follows_the_reference(single, model_cache, notes):
    """skin 0.3 A with moves of up to 0.5 A: the displacement check rebuilds the list (wrap, ghost shell, fold) on the way"""
    path = model_cache(*MODEL)
    sysm, p, hist = fr.oracle_case_run("water258", path)
    looks, res, _, _ = _minimize("water258", single, path, skin=0.3)
    assert res["rebuilds"] >= 1
    _follow("water258 skin 0.3", single, looks, res, hist, sysm.boxhi - sysm.boxlo, notes)


@PRECISIONS
def test_the_result_does_not_depend_on_how_often_the_host_looks(single, model_cache):
    path = model_cache(*MODEL)
    sysm, p, hist = fr.oracle_case_run("water30", path)
    L = sysm.boxhi - sysm.boxlo
    looks1, res1, x1, _ = _minimize("water30", single, path, maxiter=23, check_every=1)
    looks10, res10, x10, _ = _minimize("water30", single, path, maxiter=23, check_every=10)
    assert [int(g["iterations"]) for g in looks10] == [10, 20, 23]           # looks at calls 10, 20 and 24 (= maxiter + 1)
    for res in (res1, res10):
        assert res["iterations"] == 23 and res["stop"] == "maxiter"
    assert res10["force_evaluations"] == 24 and res1["force_evaluations"] == 24
    dx = x10 - x1
    dx -= L * np.round(dx / L)
    dr = x10 - hist[22]["x"]
    dr -= L * np.round(dr / L)
    print(f"check_every 10 against 1: max |dx| {np.abs(dx).max():.2e}; against the reference after 23 moves {np.abs(dr).max():.2e}")
    assert np.abs(dx).max() <= (1e-3 if single else 1e-9)
    atol, rtol = _bars(single)
    assert np.allclose(dr, 0.0, rtol, max(atol, 1e-12))
    for key in ("dt", "alpha", "uphill", "limited", "last_negative", "stop"):
        assert looks10[-1][key] == looks1[-1][key]


@PRECISIONS
def test_run_can_follow_at_once(single, model_cache):
    """after minimize: v is zero and step_no unchanged (checked in every run of this file); two step() calls give the forces and
    positions of a fresh VerletRun started from the minimised positions"""
    import torch
    from lammps_ani_amd import ani_hip, md
    path = model_cache(*MODEL)
    sysm = fr.case_system("water258")
    L = sysm.boxhi - sysm.boxlo
    _, res, xmin, (run, ani, glob) = _minimize("water258", single, path, maxiter=6, keep=True)
    assert res["iterations"] == 6
    for _ in range(2):
        run.step()
    xa, fa = glob(run.x), glob(run.f)
    assert run.step_no == 2
    ani.close()
    inp = hx.decompose(sysm, x_override=xmin)
    ani2 = ani_hip.ANI(path, 0, -1, use_single=single)
    fresh = md.VerletRun(ani2, inp, L, torch.device("cuda:0"), dt=0.1, every=7, box_lo=sysm.boxlo)
    for _ in range(2):
        fresh.step()
    tag = fresh.tag.cpu().numpy()
    xb, fb = np.zeros_like(xa), np.zeros_like(fa)
    xb[tag], fb[tag] = fresh.x[: fresh.nlocal].cpu().numpy(), fresh.f[: fresh.nlocal].cpu().numpy()
    ani2.close()
    dx = xa - xb
    dx -= L * np.round(dx / L)
    atol, rtol = _bars(single)
    print(f"two steps after minimize against a fresh loop: max |dF| {np.abs(fa - fb).max():.2e}  |dx| {np.abs(dx).max():.2e}")
    assert np.allclose(fa, fb, rtol, atol) and np.allclose(dx, 0.0, rtol, max(atol, 1e-12))
    assert np.abs(xa - xmin).max() > 0.0


def test_several_ranks_are_refused_and_so_are_unknown_parameters(model_cache, monkeypatch):
    import torch
    from lammps_ani_amd import ani_hip, md
    sysm = fr.case_system("water30")
    ani = ani_hip.ANI(model_cache(*MODEL), 0, 1)
    run = md.VerletRun(ani, hx.decompose(sysm), sysm.boxhi - sysm.boxlo, torch.device("cuda:0"), box_lo=sysm.boxlo)
    with pytest.raises(TypeError, match="unknown FIRE parameter"):
        run.minimize(0.0, 0.0, 3, dtgrowth=1.2)
    monkeypatch.setattr(run.dc, "multi", True)
    with pytest.raises(RuntimeError, match="one rank only"):
        run.minimize(0.0, 0.0, 3)
    ani.close()
