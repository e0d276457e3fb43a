"""GPU: umbrella restraints in the timestep loop (VerletRun.set_restraints / set_restraint_centres / restraint_state /
restraint_series: ani_md_restraints_* of include/ani_md.h behind every force evaluation) against the numpy reference of
tests/restraint_reference.py added to the CPU oracle, built like tests/test_npt_md.py.

The shifted 30-atom water box of tests/test_shake_md.py, where an O-H bond crosses the +x face; ANI-2x shaped model of one member.
Three restraints, centres displaced from the start values: the torsion H-O...O-H from the face-crossing hydrogen over its oxygen to
the nearest other oxygen and the hydrogen of that one which is furthest from collinear (kappa 24 kcal/mol/rad^2, +0.5 rad), the
H-O-H angle of a third molecule (kappa 60, +0.25 rad) and the distance between the oxygens of the third and a fourth molecule (kappa
150 kcal/mol/A^2, -0.4 A: a bias virial of some -150 kcal/mol, 7 000 atm in this box).  The largest bias force component of the
reference is asserted to be at least 1 kcal/mol/A.  Bars of tests/test_nvt_md.py and tests/test_npt_md.py: fp64 handle atol 1e-9,
rtol 1e-5, records rtol 1e-6; fp32 handle 1e-3.
"""
import functools

import numpy as np
import pytest

import nh_reference as nh
import npt_reference as nr
import restraint_reference as rr
import shake_reference as sr
from lammps_ani_amd import harness as hx
from test_npt_md import NPT, _records, _reference_records
from test_shake_md import _Recorder, _box, _periodic_forces

pytestmark = pytest.mark.gpu

STEPS, DT, TOL = 4, 0.5, 1e-12
PRECISIONS = pytest.mark.parametrize("single", [True, False], ids=["precision_single", "precision_double"])
KAPPA = dict(torsion=24.0, angle=60.0, distance=150.0)
SHIFT = dict(torsion=0.5, angle=0.25, distance=-0.4)


@functools.lru_cache(maxsize=None)
def _restraints():
    """the three restraints as (kind, global indices, kappa, centre), chosen on the CPU from the start positions"""
    sysm, bonds, b, _ = _box()
    x, L = sysm.x, sysm.boxhi - sysm.boxlo
    oxy = np.unique(bonds[:, 0])
    hb, ob = int(bonds[b, 1]), int(bonds[b, 0])
    d = np.sqrt((sr.minimg(x[oxy] - x[ob], L) ** 2).sum(1))
    d[oxy == ob] = np.inf
    o2 = int(oxy[np.argmin(d)])
    G = sr.minimg(x[ob] - x[o2], L)
    hs = [int(h) for o, h in bonds if o == o2]
    sin = [np.linalg.norm(np.cross(sr.minimg(x[h] - x[o2], L), G)) / np.linalg.norm(sr.minimg(x[h] - x[o2], L)) / np.linalg.norm(G) for h in hs]
    h2 = hs[int(np.argmax(sin))]
    assert max(sin) > 0.3
    rest = [int(o) for o in oxy if o not in (ob, o2)]
    o3 = rest[0]
    h3 = [int(h) for o, h in bonds if o == o3]
    d3 = np.sqrt((sr.minimg(x[rest[1:]] - x[o3], L) ** 2).sum(1))
    o4 = rest[1 + int(np.argmin(d3))]
    picks = [("torsion", (hb, ob, o2, h2)), ("angle", (h3[0], o3, h3[1])), ("distance", (o3, o4))]
    cv = rr.evaluate(x, *rr.tables([(k, ix, 0.0, 0.0) for k, ix in picks]), L)["cv"]
    return tuple((k, ix, KAPPA[k], float(cv[i]) + SHIFT[k]) for i, (k, ix) in enumerate(picks))


def _masses():
    sysm = _box()[0]
    return sr.MASSES[sysm.types - 1]


def _oracle(model_path):
    return nr.oracle_evaluator(model_path, _box()[0])


@functools.lru_cache(maxsize=None)
def _nve_reference(model_path):
    sysm, _, _, v0 = _box()
    model, lo, L = _oracle(model_path), sysm.boxlo, sysm.boxhi - sysm.boxlo

    def total(x):
        f, pe, _ = model(x, lo, L)
        fb, eb, _, _ = rr.bias(x, _restraints(), L)
        return f + fb, pe + eb

    return rr.nve_trajectory(sysm.x, v0, _masses(), total, STEPS, DT)


@functools.lru_cache(maxsize=None)
def _npt_reference(model_path, with_virial=True):
    sysm, _, _, v0 = _box()
    return nr.npt_trajectory(sysm.x, v0, _masses(), rr.biased(_oracle(model_path), _restraints(), with_virial), STEPS, DT, sysm.boxlo,
                             sysm.boxhi - sysm.boxlo, nh.T_TARGET, None, nh.T_PERIOD, p_start=nr.P_START, p_period=nr.P_PERIOD,
                             M=nh.MTCHAIN, Mp=3, fresh_k2_every_step=True)


def _loop(model_path, single, **kw):
    """(run, ani, to_global) on the shifted box with the start velocities, no restraints yet"""
    import torch
    from lammps_ani_amd import ani_hip, md
    sysm, _, _, v0 = _box()
    ani = ani_hip.ANI(model_path, 0, -1, use_single=single)
    kw.setdefault("every", 2)
    run = md.VerletRun(ani, hx.decompose(sysm), sysm.boxhi - sysm.boxlo, torch.device("cuda:0"), dt=DT, box_lo=sysm.boxlo, **kw)
    tag = run.tag.cpu().numpy()
    run.v.copy_(torch.as_tensor(np.array(v0[tag])))

    def to_global(t):
        out = np.zeros((sysm.natoms, 3))
        out[tag] = t[: run.nlocal].cpu().numpy()
        return out

    return run, ani, to_global


def _reference_now(x, L):
    return rr.evaluate(x, *rr.tables(list(_restraints())), L)


def _cv_agrees(run, x, L, what=""):
    st, ref = run.restraint_state(), _reference_now(x, L)
    assert st["nonfinite"] == 0
    assert np.allclose(st["cv"], ref["cv"], rtol=1e-12, atol=1e-12), (what, st["cv"], ref["cv"])
    assert np.allclose(st["energy"], ref["e"], rtol=1e-11, atol=1e-12) and np.isclose(st["ebias"], float(ref["E"]), rtol=1e-11)
    return st, ref


def test_the_reference_bias_is_a_force_to_reckon_with():
    sysm = _box()[0]
    ref = _reference_now(sysm.x, sysm.boxhi - sysm.boxlo)
    per = np.abs(ref["fslot"]).max(axis=(1, 2))
    print(f"largest bias force component per restraint: {per}, bias energy {float(ref['E']):.3f} kcal/mol, virial trace "
          f"{float(ref['W'][0] + ref['W'][4] + ref['W'][8]):.2f}")
    assert (per >= 1.0).all()
    (_, tors, _, _), _, _ = _restraints()
    b = _box()[2]
    assert int(_box()[1][b, 1]) == tors[0]                                 # the face-crossing hydrogen is in the torsion


@PRECISIONS
def test_four_nve_steps_follow_the_oracle_plus_restraint_reference(single, model_cache):
    path = model_cache(*nh.WATER_MODEL)
    sysm = _box()[0]
    L = sysm.boxhi - sysm.boxlo
    ref = _nve_reference(path)
    assert np.abs(_reference_now(sysm.x, L)["fslot"]).max() >= 1.0
    run, ani, glob = _loop(path, single)
    run.set_restraints(_restraints())
    atol, rtol = (1e-3, 1e-3) if single else (1e-9, 1e-5)
    builds0 = run.nbuilds
    for k in range(STEPS + 1):
        if k:
            run.step(force_rebuild=(k == 2))
        x, v, f, r = glob(run.x), glob(run.v), glob(run.f), ref[k]
        dx = x - r["x"]
        dx -= L * np.round(dx / L)
        st, now = _cv_agrees(run, x, L, f"step {k}")
        print(f"step {k} {'fp32' if single else 'fp64'}: max |dF| {np.abs(f - r['f']).max():.2e}  |dx| {np.abs(dx).max():.2e}  "
              f"|dv| {np.abs(v - r['v']).max():.2e}  pe {run.potential_energy()!r} ({r['pe']!r})  cv {st['cv']}")
        assert np.allclose(f, r["f"], rtol, atol)
        assert np.allclose(dx, 0.0, rtol, max(atol, 1e-12))
        assert np.allclose(v, r["v"], rtol, atol)
        assert np.isclose(run.potential_energy(), r["pe"], rtol=rtol, atol=atol)
        assert st["evaluations"] == 1 + k
    assert run.nbuilds == builds0 + 1
    ani.close()


@PRECISIONS
def test_four_npt_steps_with_the_bias_virial(single, model_cache):
    path = model_cache(*nh.WATER_MODEL)
    ref, without = _npt_reference(path), _npt_reference(path, False)
    atol, rtol, crtol = (1e-3, 1e-3, 1e-3) if single else (1e-9, 1e-5, 1e-6)
    # on the reference alone: leaving the bias virial out moves the record's P by more than a hundred bars
    for k in range(1, STEPS + 1):
        dp, bar = abs(ref[k]["baro"][3] - without[k]["baro"][3]), crtol * abs(ref[k]["baro"][3])
        print(f"  step {k}: P {ref[k]['baro'][3]:.1f} atm, without the bias virial {without[k]['baro'][3]:.1f}: {dp / bar:.0f} bars")
        assert dp > 100.0 * bar
    run, ani, glob = _loop(path, single, vflag=True)
    run.set_restraints(_restraints())
    run.set_npt(nh.T_TARGET, **NPT)
    for k in range(STEPS + 1):
        if k:
            run.step(force_rebuild=(k % 2 == 0))
        x, v, f, r = glob(run.x), glob(run.v), glob(run.f), ref[k]
        lo, L = run.box()
        dx = x - r["x"]
        dx -= L * np.round(dx / L)
        _cv_agrees(run, x, L, f"step {k}")                                 # in the box of the moment: the record's, not the host's
        print(f"step {k} {'fp32' if single else 'fp64'}: max |dF| {np.abs(f - r['f']).max():.2e}  |dx| {np.abs(dx).max():.2e}  "
              f"|dv| {np.abs(v - r['v']).max():.2e}  V {np.prod(L)!r} ({r['vol']!r})")
        assert np.allclose(f, r["f"], rtol, atol)
        assert np.allclose(dx, 0.0, rtol, max(atol, 1e-12))
        assert np.allclose(v, r["v"], rtol, atol)
        assert np.allclose(lo, r["lo"], rtol=crtol, atol=0.0) and np.allclose(L, r["len"], rtol=crtol, atol=0.0)
        if k:
            got, want = _records(run), _reference_records(r)
            bad = ~np.isclose(got, want, rtol=crtol, atol=0.0)
            assert not bad.any(), (np.flatnonzero(bad).tolist(), got[bad], want[bad])
            th = run.thermo()
            assert np.isclose(th["press"], r["press"], rtol=crtol, atol=crtol * abs(r["baro"][3]))
            assert np.isclose(th["pe"], r["pe"], rtol=rtol, atol=atol) and np.isclose(th["econserve"], r["econserve"], rtol=crtol)
    assert abs(ref[STEPS]["vol"] / ref[0]["vol"] - 1.0) >= 0.01
    ani.close()


@PRECISIONS
def test_nvt_with_constraints_and_where_the_launches_stand(single, model_cache):
    path = model_cache(*nh.WATER_MODEL)
    sysm, bonds, _, _ = _box()
    L = sysm.boxhi - sysm.boxlo
    run, ani, glob = _loop(path, single)
    run.set_constraints(bonds, tol=TOL)
    run.project_velocities()
    run.set_nvt(nh.T_TARGET, t_period=nh.T_PERIOD, mtchain=nh.MTCHAIN)
    run.set_restraints(_restraints())
    cl, slot = sr.build_clusters(bonds, np.arange(sysm.natoms))
    x0 = glob(run.x)
    d = np.zeros((cl.shape[0], 3))
    used = slot >= 0
    d[used] = np.sqrt((sr.minimg(x0[np.repeat(cl[:, :1], 3, 1)[used]] - x0[cl[:, 1:][used]], L) ** 2).sum(1))
    calls = []
    run._md = _Recorder(run._md, calls)
    forces = run._forces
    run._forces = lambda: (calls.append("forces"), forces())[1]
    run.run(STEPS)
    res = sr.residuals(glob(run.x), cl, d, L).max()
    assert res <= TOL + 1e-13, res
    assert run.constraint_stats()["unconverged"] == 0 and run.nvt_state()["half_steps"] == 2 * STEPS
    _cv_agrees(run, glob(run.x), L)
    mine = [c for c in calls if c == "forces" or "restraints" in c or "integrate" in c]
    assert mine == ["ani_md_nh_initial_integrate", "forces", "ani_md_restraints_eval", "ani_md_restraints_apply",
                    "ani_md_final_integrate"] * STEPS, mine
    ani.close()


@PRECISIONS
def test_cleared_restraints_leave_the_loop_as_it_was(single, model_cache):
    path = model_cache(*nh.WATER_MODEL)
    sysm = _box()[0]
    out = []
    for touch in (False, True):
        run, ani, glob = _loop(path, single)
        _periodic_forces(run, sysm)
        if touch:
            run.set_restraints(_restraints(), stride=1)
            assert run.restraint_state()["evaluations"] == 1
            run.set_restraints([])
            with pytest.raises(RuntimeError, match="no restraints"):
                run.restraint_state()
        calls = []
        run._md = _Recorder(run._md, calls)
        run.run(20)
        out.append((calls, glob(run.x), glob(run.v), glob(run.f), run.potential_energy()))
        ani.close()
    (ca, xa, va, fa, ea), (cb, xb, vb, fb, eb) = out
    assert ca == cb and not any("restraints" in c for c in cb) and cb.count("ani_md_final_initial_integrate") == 19
    assert xa.tobytes() == xb.tobytes() and va.tobytes() == vb.tobytes() and fa.tobytes() == fb.tobytes() and ea == eb


@PRECISIONS
def test_the_series(single, model_cache):
    """the restraint kernels are fp64 whatever the handle: the same 1e-12 on both"""
    path = model_cache(*nh.WATER_MODEL)
    sysm = _box()[0]
    L = sysm.boxhi - sysm.boxlo
    run, ani, glob = _loop(path, single)
    run.set_restraints(_restraints(), stride=2, capacity=8)
    want = [(0, _reference_now(glob(run.x), L))]
    calls = []
    run._md = _Recorder(run._md, calls)
    for k in range(1, 8):
        run.run(1)
        if k % 2 == 0:
            want.append((k, _reference_now(glob(run.x), L)))
    assert "ani_md_final_initial_integrate" not in calls and calls.count("ani_md_restraints_apply") == 7
    s = run.restraint_series()
    assert s["step"].tolist() == [0, 2, 4, 6] and s["dropped"] == 0 and s["cv"].shape == (4, 3) == s["ebias"].shape
    for row, (k, ref) in enumerate(want):
        assert np.allclose(s["cv"][row], ref["cv"], rtol=1e-12, atol=0.0) and np.allclose(s["ebias"][row], ref["e"], rtol=1e-12, atol=0.0), k
    assert run.restraint_series(reset=True)["step"].tolist() == [0, 2, 4, 6]
    s = run.restraint_series()
    assert s["step"].shape == (0,) and s["cv"].shape == (0, 3) and s["dropped"] == 0
    run.run(3)                                                             # steps 8, 9, 10 in one call: the boundary launch stays
    assert run.restraint_series()["step"].tolist() == [8, 10]
    ani.close()
    # a buffer of two rows keeps the last two and counts the rest
    run, ani, glob = _loop(path, single)
    run.set_restraints(_restraints(), stride=2, capacity=2)
    for _ in range(7):
        run.run(1)
    s = run.restraint_series()
    assert s["step"].tolist() == [4, 6] and s["dropped"] == 2
    ref = _reference_now(glob(run.x), L)
    assert np.allclose(run.restraint_state()["cv"], ref["cv"], rtol=1e-12, atol=0.0)
    # moving the windows: no new row, the forces are evaluated again
    cen = [r[3] for r in _restraints()]
    f_before = glob(run.f)
    run.set_restraint_centres([c + 0.1 for c in cen])
    assert run.restraint_series()["step"].tolist() == [4, 6] and np.abs(glob(run.f) - f_before).max() > 0.1
    run.set_restraint_centres(cen, kappas=[0.0, 0.0, 0.0])
    assert run.restraint_state()["ebias"] == 0.0
    # stride 0: nothing is recorded
    run.set_restraints(_restraints())
    run.run(2)
    assert run.restraint_series()["step"].shape == (0,)
    ani.close()


@PRECISIONS
def test_minimize_with_restraints(single, model_cache):
    path = model_cache(*nh.WATER_MODEL)
    sysm = _box()[0]
    lo, L = sysm.boxlo, sysm.boxhi - sysm.boxlo
    run, ani, glob = _loop(path, single)
    run.set_restraints(_restraints(), stride=1)
    d0 = abs(run.restraint_state()["cv"][2] - _restraints()[2][3])
    res = run.minimize(0.0, 0.0, 30)
    st = run.restraint_state()
    x = glob(run.x)
    _, pe, _ = _oracle(path)(x, lo, L)
    atol, rtol = (1e-3, 1e-3) if single else (1e-9, 1e-5)
    d1 = abs(st["cv"][2] - _restraints()[2][3])
    print(f"  minimize: {res['iterations']} iterations, |f| {res['fnorm_before']:.2f} -> {res['fnorm_after']:.2f}, |D| of the distance {d0:.4f} -> "
          f"{d1:.4f}, pe - bias {run.potential_energy() - st['ebias']!r} (oracle {pe!r})")
    assert np.isclose(run.potential_energy() - st["ebias"], pe, rtol=rtol, atol=atol)
    assert res["fnorm_after"] < res["fnorm_before"] and d1 < d0 and res["iterations"] == 30
    assert st["evaluations"] == 1 + res["force_evaluations"]
    assert run.restraint_series()["step"].tolist() == [0]                  # minimize does not sample
    ani.close()


@PRECISIONS
def test_where_it_raises(single, model_cache, monkeypatch):
    path = model_cache(*nh.WATER_MODEL)
    run, ani, _ = _loop(path, single)
    good = list(_restraints())
    tors = good[0][1]
    for bad, word in (([("bond", (0, 1), 1.0, 1.0)], "unknown kind"), ([("distance", (0, 999), 1.0, 1.0)], r"unknown tag 999"),
                      ([("torsion", (tors[0], tors[1], tors[0], tors[3]), 1.0, 1.0)], "repeated tag"),
                      ([("angle", (0, 1), 1.0, 1.0)], "takes 3 tags"), ([("distance", (0, 1, 2), 1.0, 1.0)], "takes 2 tags"),
                      ([("torsion", (0, 1, 2), 1.0, 1.0)], "takes 4 tags"), ([("distance", (0, 1), -1.0, 1.0)], "kappa"),
                      ([("distance", (0, 1), float("nan"), 1.0)], "kappa"), ([("distance", (0, 1), float("inf"), 1.0)], "kappa"),
                      ([("distance", (0, 1), 1.0, float("nan"))], "centre"), ([("distance", (0, 1), 1.0, float("inf"))], "centre")):
        with pytest.raises(ValueError, match=word):
            run.set_restraints(good + bad)
        assert run._restr is None
    with pytest.raises(ValueError, match="stride"):
        run.set_restraints(good, stride=-1)
    with pytest.raises(ValueError, match="capacity"):
        run.set_restraints(good, stride=1, capacity=0)
    for name in ("restraint_state", "restraint_series"):
        with pytest.raises(RuntimeError, match="no restraints"):
            getattr(run, name)()
    with pytest.raises(RuntimeError, match="no restraints"):
        run.set_restraint_centres([1.0, 1.0, 1.0])
    run.set_restraints(good)
    with pytest.raises(ValueError, match="3 restraints"):
        run.set_restraint_centres([1.0, 1.0])
    with pytest.raises(ValueError, match="kappa"):
        run.set_restraint_centres([1.0, 1.0, 1.0], kappas=[1.0, -1.0, 1.0])
    with pytest.raises(ValueError, match="centre"):
        run.set_restraint_centres([1.0, float("nan"), 1.0])
    run.set_restraints([])
    monkeypatch.setattr(run.dc, "multi", True)                             # what a loop on two ranks sees
    with pytest.raises(RuntimeError, match="one rank only"):
        run.set_restraints(good)
    monkeypatch.setattr(run.dc, "multi", False)
    monkeypatch.setattr(run, "_native_rebuild", False)
    with pytest.raises(RuntimeError, match="native re-neighbouring"):
        run.set_restraints(good)
    monkeypatch.setattr(run, "_native_rebuild", True)
    # a restraint that is not finite (the two oxygens of the distance on one point; the model is kept out of it by the elementwise
    # calculator of tests/test_shake_md.py): the energy is NaN and the loop's look raises
    _periodic_forces(run, _box()[0])
    run.set_restraints(good)
    local = run.tag.cpu().numpy().tolist()
    run.x[local.index(good[2][1][0])] = run.x[local.index(good[2][1][1])]
    run._ghosts_and_forces(False)
    st = run.restraint_state()
    assert st["nonfinite"] == 1 and np.isnan(st["ebias"]) and np.isnan(st["energy"][2]) and np.isfinite(st["energy"][:2]).all()
    with pytest.raises(RuntimeError, match="non-finite energy"):
        run._look()
    ani.close()
