"""GPU: the Nose-Hoover chain in the timestep loop (VerletRun.set_nvt / nvt_state / thermo: ani_md_nh_* and ani_md_thermo of
include/ani_md.h around the integrator) against the numpy thermostatted velocity Verlet of tests/nh_reference.py with the CPU oracle
as its calculator, built like tests/test_shake_md.py.

The reference's 30-atom water box, ANI-2x shaped model of one member, velocities from a numpy draw at 300 K with the momentum
removed, target 600 K, t_period 20 fs, three links.  Trajectory bars of tests/test_trajectory_vs_oracle.py (fp64 handle atol 1e-9,
rtol 1e-5; fp32 handle 1e-3 / 1e-3); the chain record, whose only input is K2, at rtol 1e-6 / 1e-3.
"""
import functools
import os

import numpy as np
import pytest

import nh_reference as nh
import shake_reference as sr
from lammps_ani_amd import harness as hx
from test_shake_md import _Recorder, _periodic_forces

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, DT = 4, 0.5
PRECISIONS = pytest.mark.parametrize("single", [True, False], ids=["precision_single", "precision_double"])


@functools.lru_cache(maxsize=None)
def _reference(model_path):
    s, m, v0 = nh.water30(ROOT)
    return nh.nvt_trajectory(s.x, v0, m, nh.oracle_evaluator(model_path, s), STEPS, DT, nh.T_TARGET, None, nh.T_PERIOD, nh.MTCHAIN)


def _loop(model_path, single, dt=DT, velocities=True, **kw):
    """(run, ani, to_global) on the box with the start velocities"""
    import torch
    from lammps_ani_amd import ani_hip, md
    s, _, v0 = nh.water30(ROOT)
    ani = ani_hip.ANI(model_path, 0, -1, use_single=single)
    kw.setdefault("every", 2)
    run = md.VerletRun(ani, hx.decompose(s), s.boxhi - s.boxlo, torch.device("cuda:0"), dt=dt, box_lo=s.boxlo, **kw)
    tag = run.tag.cpu().numpy()
    if velocities:
        run.v.copy_(torch.as_tensor(np.array(v0[tag])))

    def to_global(t):
        out = np.zeros((s.natoms, 3))
        out[tag] = t[: run.nlocal].cpu().numpy()
        return out

    return run, ani, to_global


@PRECISIONS
def test_four_thermostatted_steps_follow_the_oracle_driven_reference(single, model_cache):
    path = model_cache(*nh.WATER_MODEL)
    s, m, _ = nh.water30(ROOT)
    L = s.boxhi - s.boxlo
    ref = _reference(path)
    run, ani, glob = _loop(path, single)
    run.set_nvt(nh.T_TARGET, t_period=nh.T_PERIOD, mtchain=nh.MTCHAIN)
    atol, rtol, crtol = (1e-3, 1e-3, 1e-3) if single else (1e-9, 1e-5, 1e-6)
    builds0 = run.nbuilds
    for k in range(STEPS + 1):
        if k:
            run.step(force_rebuild=(k % 2 == 0))
        x, v, f, r = glob(run.x), glob(run.v), glob(run.f), ref[k]
        dx = x - r["x"]
        dx -= L * np.round(dx / L)                       # the loop wraps owned atoms into the box at a re-neighbouring
        st = run.nvt_state()
        rec = r["chain"]
        print(f"step {k} {'fp32' if single else 'fp64'}: max |dF| {np.abs(f - r['f']).max():.2e}  |dx| {np.abs(dx).max():.2e}  "
              f"|dv| {np.abs(v - r['v']).max():.2e}  s {st['s']!r} ({rec[2]!r})  ecouple {st['ecouple']!r} ({rec[4]!r})")
        assert np.allclose(f, r["f"], rtol, atol)
        assert np.allclose(dx, 0.0, rtol, max(atol, 1e-12))
        assert np.allclose(v, r["v"], rtol, atol)
        assert st["half_steps"] == 2 * k and st["nonfinite"] == 0
        if k:
            assert st["t_target"] == nh.T_TARGET and st["tdof"] == 3 * 30 - 3
            got = np.concatenate([[st["k2"], st["s"], st["ecouple"]], st["eta"], st["eta_dot"], st["eta_dotdot"]])
            want = np.concatenate([rec[[1, 2, 4]], rec[8:8 + 3], rec[16:16 + 3], rec[24:24 + 3]])
            assert np.allclose(got, want, rtol=crtol, atol=0.0), (got, want)
    assert run.nbuilds == builds0 + 2
    assert abs(ref[STEPS]["ke"] - ref[0]["ke"]) > 0.5            # the thermostat acted: the box was heated
    ani.close()


def test_conserved_quantity_with_run(model_cache):
    """The two conditions of tests/test_nh_reference_cpu.py on the device (fp64 handle, run()): 50 fs as 100 steps of 0.5 fs and as
    200 of 0.25 fs, thermo() read every femtosecond (run(2) / run(4): the same instants in both).  Reference, sampled the same way:
    0.151 and 0.042 kcal/mol, ratio 0.28; pe + ke moves by 97."""
    path = model_cache(*nh.WATER_MODEL)
    w = {}
    for dt, chunk in ((0.5, 2), (0.25, 4)):
        run, ani, _ = _loop(path, False, dt=dt, every=10)
        run.set_nvt(nh.T_TARGET, t_period=nh.T_PERIOD, mtchain=nh.MTCHAIN)
        rows = [run.thermo()]
        for _ in range(50):
            run.run(chunk)
            rows.append(run.thermo())
        e = np.array([r["etotal"] for r in rows])
        c = np.array([r["econserve"] for r in rows])
        w[dt] = (nh.wander(c), nh.wander(e))
        assert run.step_no == 50 * chunk and run.nvt_state()["half_steps"] == 100 * chunk
        assert all(np.isclose(r["econserve"], r["etotal"] + r["ecouple"], rtol=1e-14) for r in rows)
        ani.close()
    print(f"wander of pe + ke + ecouple: {w[0.5][0]:.4f} (dt 0.5), {w[0.25][0]:.4f} (dt 0.25), ratio {w[0.25][0] / w[0.5][0]:.3f}; "
          f"of pe + ke: {w[0.5][1]:.2f}, {w[0.25][1]:.2f}")
    assert w[0.25][0] <= 0.5 * w[0.5][0]
    for dt in (0.5, 0.25):
        assert w[dt][0] <= 0.01 * w[dt][1]


def test_run_agrees_with_steps_and_the_ramp_ends_on_t_stop(model_cache):
    """run(N) carries K2 through the chain's own scaling, step() sums it again: equal to the rounding of K2.  With the model as the
    calculator two runs of the same loop already differ by the arrival order of its floating-point atomics (tests/test_shake_md.py),
    so the comparison is made with the elementwise calculator of that test."""
    path = model_cache(*nh.WATER_MODEL)
    s, _, _ = nh.water30(ROOT)
    out = []
    for stepwise in (False, True):
        run, ani, glob = _loop(path, False)
        _periodic_forces(run, s)
        run.set_nvt(nh.T_TARGET, t_period=nh.T_PERIOD, mtchain=nh.MTCHAIN)
        if stepwise:
            for _ in range(12):
                run.step()
        else:
            run.run(12)
        out.append((glob(run.v), glob(run.x), run.nvt_state()))
        ani.close()
    (va, xa, sa), (vb, xb, sb) = out
    print(f"run(12) against 12 step(): max |dv| / |v| {np.abs(va - vb).max() / np.abs(va).max():.2e}")
    assert np.allclose(va, vb, rtol=1e-12, atol=1e-12 * np.abs(va).max()) and np.allclose(xa, xb, rtol=1e-12, atol=1e-12)
    assert sa["half_steps"] == sb["half_steps"] == 24 and np.isclose(sa["ecouple"], sb["ecouple"], rtol=1e-10)
    # a ramp: step k of run(N) has the target t_start + k / N (t_stop - t_start), the record keeps the last one
    run, ani, _ = _loop(path, False)
    _periodic_forces(run, s)
    run.set_nvt(300.0, 600.0, t_period=nh.T_PERIOD)
    assert run.nvt_state()["t_target"] == 0.0 and run.nvt_state()["half_steps"] == 0
    run.run(1)
    assert run.nvt_state()["t_target"] == 600.0
    run.run(7)
    assert run.nvt_state()["t_target"] == 600.0 and run.nvt_state()["half_steps"] == 16
    run.step()
    assert run.nvt_state()["t_target"] == 600.0                   # afterwards the target stays at t_stop
    seen = []
    rec = _Recorder(run._md, [])
    real = run._md.ani_md_nh_chain
    run._md = rec
    rec.ani_md_nh_chain = lambda *a: (seen.append((a[2], a[3])), real(*a))[1]
    run.run(4)
    assert [t for _, t in seen] == [375.0, 375.0, 450.0, 450.0, 525.0, 525.0, 600.0, 600.0]
    assert [bool(p) for p, _ in seen] == [True, True, False, True, False, True, False, True]   # only the first reads fresh partials
    ani.close()


@PRECISIONS
def test_thermostat_with_all_bonds_constrained(single, model_cache):
    path = model_cache(*nh.WATER_MODEL)
    s, _, _ = nh.water30(ROOT)
    L = s.boxhi - s.boxlo
    bonds = sr.water_oh_bonds(s)
    run, ani, glob = _loop(path, single, vflag=True)
    run.set_nvt(nh.T_TARGET, t_period=nh.T_PERIOD, mtchain=nh.MTCHAIN)
    assert np.isfinite(run.thermo()["press"])                     # with vflag and no constraints there is a pressure
    run.set_constraints(bonds, tol=1e-12)                         # after set_nvt: the degrees of freedom follow
    run.project_velocities()
    cl, slot = sr.build_clusters(bonds, np.arange(s.natoms))
    x0 = glob(run.x)
    d = np.zeros((len(cl), 3))
    for k in range(3):
        u = cl[:, 1 + k] >= 0
        r = sr.minimg(x0[cl[u, 0]] - x0[cl[u, 1 + k]], L)
        d[u, k] = np.sqrt((r * r).sum(1))
    calls = []
    run._md = _Recorder(run._md, calls)
    for k in range(4):
        if k < 2:
            run.step(force_rebuild=(k == 1))
        else:
            run.run(1)
        x, v = glob(run.x), glob(run.v)
        res, defect = sr.residuals(x, cl, d, L).max(), sr.velocity_defect(x, v, cl, L)
        st = run.nvt_state()
        print(f"step {k + 1} {'fp32' if single else 'fp64'}: residual {res:.2e}  |r.dv|/|r| {defect:.2e}  s {st['s']!r}  tdof {st['tdof']}")
        assert res <= 1e-12 + 1e-13, res
        assert defect <= 1e-12 * np.abs(v).max(), defect
        assert st["tdof"] == 3 * 30 - 3 - 20 and st["half_steps"] == 2 * (k + 1) and st["s"] != 1.0
    order = [c for c in calls if c.startswith("ani_md_nh_") or "integrate" in c or "shake" in c or "rattle" in c]
    assert order[:10] == ["ani_md_nh_kinetic", "ani_md_nh_chain", "ani_md_nh_initial_integrate", "ani_md_shake_positions",
                          "ani_md_final_integrate", "ani_md_rattle_velocities", "ani_md_nh_kinetic", "ani_md_nh_chain", "ani_md_nh_scale",
                          "ani_md_nh_kinetic"]
    th = run.thermo()
    assert np.isnan([th[k] for k in ("press", "pxx", "pyy", "pzz", "pxy", "pxz", "pyz")]).all()
    assert np.isclose(th["temp"], run.temperature(30), rtol=1e-12)
    ani.close()


@PRECISIONS
def test_thermo_record_of_the_loop(single, model_cache):
    path = model_cache(*nh.WATER_MODEL)
    s, m, _ = nh.water30(ROOT)
    vol = float(np.prod(s.boxhi - s.boxlo))
    run, ani, _ = _loop(path, single, vflag=True)
    for thermostat in (False, True):
        if thermostat:
            run.set_nvt(nh.T_TARGET, t_period=nh.T_PERIOD)
        run.run(3)
        th = run.thermo()
        ke, pe, W = run.kinetic_energy(), run.potential_energy(), run.virial()
        assert np.isclose(th["ke"], ke, rtol=1e-12) and th["pe"] == pe and np.isclose(th["temp"], run.temperature(30), rtol=1e-12)
        assert np.isclose(th["etotal"], pe + ke, rtol=1e-12) and th["vol"] == vol
        assert np.isclose(th["density"], m.sum() / 0.602214129 / vol, rtol=1e-12) and 0.5 < th["density"] < 1.5
        ec = run.nvt_state()["ecouple"] if thermostat else 0.0
        assert th["ecouple"] == ec and np.isclose(th["econserve"], pe + ke + ec, rtol=1e-12) and (ec != 0.0) == thermostat
        v = run.v.cpu().numpy()
        mass = run.mass[:, 0].cpu().numpy()
        K = nh.MVV2E * np.einsum("i,ia,ib->ab", mass, v, v)
        P = (K + W) / vol * nh.NKTV2P
        scale = np.abs(K).max() + np.abs(W).max()
        want = [np.trace(P) / 3.0, P[0, 0], P[1, 1], P[2, 2], P[0, 1], P[0, 2], P[1, 2]]
        got = [th[k] for k in ("press", "pxx", "pyy", "pzz", "pxy", "pxz", "pyz")]
        print(f"  thermo {'fp32' if single else 'fp64'} nvt {thermostat}: press {th['press']:.3f} atm, temp {th['temp']:.3f} K, "
              f"econserve {th['econserve']:.6f}")
        assert np.allclose(got, want, rtol=0.0, atol=1e-12 * scale / vol * nh.NKTV2P), (got, want)
    ani.close()
    run, ani, _ = _loop(path, single)                             # without vflag: no pressure
    th = run.thermo()
    assert np.isnan([th[k] for k in ("press", "pxx", "pyy", "pzz", "pxy", "pxz", "pyz")]).all() and np.isfinite(th["etotal"])
    ani.close()


@PRECISIONS
def test_cleared_thermostat_leaves_the_loop_as_it_was(single, model_cache):
    """set_nvt(None) after set_nvt(T): run(20) makes the launches of a loop that never had a thermostat and, with the elementwise
    calculator of tests/test_shake_md.py (the model's force kernels add in arrival order), ends bitwise where that loop ends."""
    path = model_cache(*nh.WATER_MODEL)
    s, _, v0 = nh.water30(ROOT)
    out = []
    for touch in (False, True):
        import torch
        run, ani, glob = _loop(path, single)
        _periodic_forces(run, s)
        if touch:
            run.set_nvt(nh.T_TARGET, t_period=nh.T_PERIOD)
            run.set_nvt(None)
            with pytest.raises(RuntimeError, match="no thermostat"):
                run.nvt_state()
        calls = []
        run._md = _Recorder(run._md, calls)
        run.run(20)
        out.append((calls, glob(run.x), glob(run.v), glob(run.f)))
        ani.close()
    (ca, xa, va, fa), (cb, xb, vb, fb) = out
    assert ca == cb and not any("_nh_" in c for c in cb) and cb.count("ani_md_final_initial_integrate") == 19
    assert xa.tobytes() == xb.tobytes() and va.tobytes() == vb.tobytes() and fa.tobytes() == fb.tobytes()
    assert np.abs(va - v0).max() > 1e-4                           # the run moved


def test_where_it_raises(model_cache, monkeypatch):
    import torch
    from lammps_ani_amd import ani_hip, md
    path = model_cache(*nh.WATER_MODEL)
    run, ani, _ = _loop(path, True)
    for bad in ((0.0,), (-5.0,), (300.0, 0.0), (float("nan"),)):
        with pytest.raises(ValueError, match="positive"):
            run.set_nvt(*bad)
    for M in (0, 9):
        with pytest.raises(ValueError, match="mtchain"):
            run.set_nvt(300.0, mtchain=M)
    with pytest.raises(RuntimeError, match="no thermostat"):
        run.nvt_state()
    run.set_nvt(300.0)
    assert run._nvt["par"].t_period == 100.0 * run.dt and run._nvt["t_stop"] == 300.0
    assert run.minimize(0.0, 0.0, 2)["iterations"] == 2 and run.nvt_state()["half_steps"] == 0    # minimize leaves the chain alone
    monkeypatch.setattr(run.dc, "multi", True)                    # what a loop on two ranks sees
    with pytest.raises(RuntimeError, match="one rank only"):
        run.set_nvt(300.0)
    with pytest.raises(RuntimeError, match="one rank"):
        run.thermo()
    monkeypatch.setattr(run.dc, "multi", False)
    ani.close()
    s, _, _ = nh.water30(ROOT)
    ani = ani_hip.ANI(path, 0, -1, use_single=True)
    run = md.VerletRun(ani, hx.decompose(s), s.boxhi - s.boxlo, torch.device("cuda:0"), dt=DT, box_lo=s.boxlo, langevin=(300.0, 100.0))
    with pytest.raises(RuntimeError, match="Langevin"):
        run.set_nvt(300.0)
    ani.close()
