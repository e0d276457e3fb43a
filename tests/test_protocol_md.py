"""GPU: per-atom masses, momentum removal and recentring in the timestep loop (VerletRun atom_masses / com_state / zero_momentum /
create_velocities(rot=True) / set_momentum / set_recenter: the kernels of include/ani_md_protocol.h), on the reference's 30-atom
water box, tests/golden/water-0.8nm.data.

Where a comparison is bitwise the calculator is the elementwise one of tests/test_shake_md.py (the atoms do not interact, the same
positions give the same bits); its force law conserves neither momentum nor angular momentum, so the momentum fix has work to do.
Launch parity after clearing, per-atom masses, momentum and recentring with the model in both precisions, the refusals.
"""
import os

import numpy as np
import pytest

import md_loop_reference as mr
import nh_reference as nh
import protocol_reference as pr
from test_nvt_md import _loop
from test_shake_md import _Recorder, _periodic_forces

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.5
DRIFT = np.array([0.4, -0.4, 0.4])
PRECISIONS = pytest.mark.parametrize("single", [True, False], ids=["precision_single", "precision_double"])


def _elementwise(model_cache, **kw):
    s, _, _ = nh.water30(ROOT)
    run, ani, glob = _loop(model_cache(*nh.WATER_MODEL), True, **kw)
    _periodic_forces(run, s)
    return run, ani, glob, s


def _force_law(s):
    lo, L = s.boxlo, s.boxhi - s.boxlo
    phase = np.arange(s.natoms, dtype=np.float64)[:, None]
    return lambda x: 30.0 * np.sin(2.0 * np.pi * (x - lo) / L + phase)


def _state(run, glob):
    return glob(run.x).tobytes(), glob(run.v).tobytes()


# ---- launch parity after clearing -----------------------------------------------------------------------------------------
def _trace(run):
    calls = []
    md = run._md
    run._md = _Recorder(md, calls)
    for k in range(3):
        run.step(force_rebuild=(k == 1))
    run.run(3)
    run._md = md
    return [c[len("ani_md_"):] for c in calls]


def test_cleared_features_leave_the_launches_and_the_trajectory_of_a_loop_that_never_had_them(model_cache):
    run, ani, glob, _ = _elementwise(model_cache, every=1)
    plain = _trace(run)
    run.run(20)
    end = _state(run, glob)
    ani.close()
    assert not any("com_" in c for c in plain)
    run, ani, glob, _ = _elementwise(model_cache, every=1)
    start = _state(run, glob)
    run.set_images()
    run.set_momentum(2, angular=True)
    run.set_recenter((0.5, None, 0.5))
    run.set_momentum(0)
    run.set_recenter(None)
    run.set_images(False)
    assert _state(run, glob) == start and run._mom is None and run._recenter is None
    assert _trace(run) == plain
    run.run(20)
    assert _state(run, glob) == end
    # and while they are set, they launch: sample + apply for each fix, the one-launch boundary kept where no fix stands behind a step
    run.set_images()
    run.set_momentum(2, angular=True)
    run.set_recenter((0.5, None, 0.5))
    on = _trace(run)
    assert on.count("final_integrate") + on.count("final_initial_integrate") == 6 and on.count("final_initial_integrate") == 1
    assert on.count("com_sample") == on.count("com_apply") == 6 + 3               # recentring every step, momentum on steps 2, 4, 6 of six
    ani.close()


# ---- per-atom masses -------------------------------------------------------------------------------------------------
def test_atom_masses_equal_to_the_species_masses_change_nothing(model_cache):
    from lammps_ani_amd import harness as hx
    s, m, _ = nh.water30(ROOT)
    inp = hx.decompose(s)
    by_owned = m[np.asarray(inp.tag[: inp.nlocal])]                           # the order of the owned atoms of the loop's input
    out = []
    for given in (False, True):
        run, ani, glob, _ = _elementwise(model_cache, **({"atom_masses": by_owned} if given else {}))
        assert (run.tag.cpu().numpy() == np.asarray(inp.tag[: inp.nlocal])).all()
        run.run(20)
        out.append(_state(run, glob))
        ani.close()
    assert out[0] == out[1]


def test_hydrogen_mass_repartitioning(model_cache):
    s, m, v0 = nh.water30(ROOT)
    hydrogen = m < 2.0
    hmr = np.where(hydrogen, 3.0 * m, m - 2.0 * 2.0 * m[hydrogen][0])          # every oxygen gives 2 x 1.008 to each of its two hydrogens
    assert abs(hmr.sum() - m.sum()) <= 1e-12 * m.sum() and (hmr > 0).all() and hydrogen.sum() == 20
    plain, ani0, _, _ = _elementwise(model_cache)
    density = plain.thermo()["density"]
    ani0.close()
    from lammps_ani_amd import harness as hx
    inp = hx.decompose(s)
    run, ani, glob, _ = _elementwise(model_cache, atom_masses=hmr[np.asarray(inp.tag[: inp.nlocal])])
    got = run.thermo()["density"]
    assert abs(got - density) <= 1e-12 * density
    L = s.boxhi - s.boxlo
    assert abs(density - m.sum() / np.prod(L) / 0.602214129) <= 1e-12 * density
    t_np = 2.0 * pr.kinetic(hmr, v0) / ((3 * 30 - 3) * pr.BOLTZ)
    assert abs(run.temperature(30) - t_np) <= 1e-12 * t_np
    assert abs(run.temperature(30) - 2.0 * pr.kinetic(m, v0) / (87 * pr.BOLTZ)) > 0.1 * t_np      # the masses do count
    force = _force_law(s)
    dtfm = (0.5 * DT * pr.FTM2V) / hmr
    x1, vh, _ = mr.initial_integrate(s.x, v0, force(s.x), dtfm, DT, s.x, 0.0)
    v1, _ = mr.final_integrate(vh, force(x1), dtfm)
    run.step()
    ex, ev = np.abs(glob(run.x) - x1).max(), np.abs(glob(run.v) - v1).max()
    print(f"one step with HMR masses: |dx| {ex:.2e} A, |dv| {ev:.2e} A/fs")
    assert ex <= 1e-13 * np.abs(x1).max() and ev <= 1e-13 * np.abs(v1).max()      # the REL of tests/test_md_loop_kernels.py
    v_plain = mr.final_integrate(mr.initial_integrate(s.x, v0, force(s.x), (0.5 * DT * pr.FTM2V) / m, DT, s.x, 0.0)[1], force(x1),
                                 (0.5 * DT * pr.FTM2V) / m)[0]
    assert np.abs(v1 - v_plain).max() > 1e-6
    ani.close()


# ---- momentum and recentring ----------------------------------------------------------------------------------------------
def _momenta(run, glob, m, s):
    """(|P| [3], |L| [3], bounds) of the loop's state by the reference's own sample of the downloaded arrays.  The bounds: a state that
    a sample and an apply have just cleaned, with the record of that sample gone -- its angular momentum is bounded by the sums of
    magnitudes of this state (the removal takes a part away and a rescale stays near 1: a factor 2 covers both)."""
    L = s.boxhi - s.boxlo
    x, v = run.unwrapped_positions(), glob(run.v)
    rec, terms = pr.com_sample(x, None, v, m, s.boxlo + 0.5 * L, L, 0)
    b = pr.com_bounds(rec, terms)
    depth = 30 / 256.0 + 24.0
    I6 = rec[pr.C_INERTIA:pr.C_INERTIA + 6]
    I = np.array([[I6[0], I6[3], I6[4]], [I6[3], I6[1], I6[5]], [I6[4], I6[5], I6[2]]])
    cond, big = np.linalg.cond(I), 3.0 * np.abs(I).max()
    w = cond / np.abs(I).max() * terms["al"].max()
    bound_p = 2.0 * (2.0 * terms["aM"] * b["vcm"] + (depth + 1.0) * pr.EPS * terms["ap"])
    bound_l = 2.0 * (2.0 * b["angmom"] + 3.0 * b["inertia"].max() * w + 38.0 * pr.EPS * cond * big * w)
    return rec[pr.C_MASS] * np.abs(rec[pr.C_VCM:pr.C_VCM + 3]), np.abs(rec[pr.C_ANGMOM:pr.C_ANGMOM + 3]), bound_p, bound_l, terms


def test_create_velocities_with_rot_leaves_no_momentum(model_cache):
    s, m, _ = nh.water30(ROOT)
    run, ani, glob = _loop(model_cache(*nh.WATER_MODEL), True, velocities=False)
    with pytest.raises(RuntimeError, match="set_images"):
        run.create_velocities(300.0, rot=True)
    run.set_images()
    run.create_velocities(300.0)
    P0, L0, _, _, _ = _momenta(run, glob, m, s)
    run.create_velocities(300.0, rot=True)
    P, Lr, bp, bl, terms = _momenta(run, glob, m, s)
    print(f"mom yes alone: |L| {L0.max():.3e}; rot yes: |P| {P.max():.3e} (bound {bp.min():.3e}), |L| {Lr.max():.3e} (bound {bl.min():.3e})")
    assert (P <= bp).all() and (Lr <= bl).all()
    assert L0.max() > 1e6 * bl.max()                                        # without rot the angular momentum is there
    assert abs(run.temperature(30) - 300.0) <= 1e-9
    st = run.com_state()
    assert st["count"] == 30 and st["singular"] == 0 and st["nonfinite"] == 0 and abs(st["mass"] - m.sum()) <= 1e-12 * m.sum()
    ani.close()


@PRECISIONS
def test_recenter_holds_the_centre_of_mass_under_a_drift(single, model_cache):
    import torch
    s, m, v0 = nh.water30(ROOT)
    L = s.boxhi - s.boxlo
    centre = s.boxlo + 0.5 * L
    ends = {}
    for recentred in (True, False):
        run, ani, glob = _loop(model_cache(*nh.WATER_MODEL), single, velocities=False)
        run.v.copy_(torch.as_tensor((v0 + DRIFT)[run.tag.cpu().numpy()]))
        run.set_images()
        first = run.com_state()["xcm"]
        if recentred:
            run.set_recenter((0.5, 0.5, 0.5))
        builds0, worst = run.nbuilds, 0.0
        for k in range(60):
            # one re-neighbouring for certain: the shift cancels the drift, so the displacement check may never ask for one in 30 fs
            run.step(force_rebuild=(k == 30))
            if recentred:
                worst = max(worst, float(np.abs(run.com_state()["xcm"] - centre).max()))
        ends[recentred] = run.com_state()["xcm"] - first
        if recentred:
            print(f"{'fp32' if single else 'fp64'} handle: largest |XCM - centre| over 60 steps {worst:.2e} A, "
                  f"{run.nbuilds - builds0} re-neighbourings (one of them forced)")
            assert worst <= 1e-10
            assert run.nbuilds - builds0 >= 1
            assert run.com_state()["nonfinite"] == 0
            # the forces of the last step against a forced rebuild at the same positions: the list that the shifts went through
            # is as good as a fresh one (the bars that tests/test_nvt_md.py holds a step of the loop to)
            f_loop = glob(run.f)
            run._ghosts_and_forces(True)
            f_new = glob(run.f)
            atol, rtol = (1e-3, 1e-3) if single else (1e-9, 1e-5)
            print(f"  forces kept list against rebuilt: largest difference {np.abs(f_loop - f_new).max():.2e} kcal/mol/A")
            assert np.allclose(f_loop, f_new, rtol=rtol, atol=atol)
        ani.close()
    print(f"  unrecentred: XCM moved {ends[False]}")
    assert np.abs(np.abs(ends[False]) - 12.0).max() <= 1e-3 and (np.sign(ends[False]) == np.sign(DRIFT)).all()


def test_fix_momentum_every_fifth_step(model_cache):
    s, m, _ = nh.water30(ROOT)
    out = []
    for stepped in (True, False):
        run, ani, glob, _ = _elementwise(model_cache)
        run.set_images()
        run.set_momentum(5, angular=True)
        if stepped:
            for k in range(1, 21):
                run.step()
                P, Lr, bp, bl, _ = _momenta(run, glob, m, s)
                if k % 5 == 0:
                    assert (P <= bp).all() and (Lr <= bl).all(), (k, P, bp, Lr, bl)
                elif k % 5 == 2:
                    assert P.max() > 1e6 * bp.max() and Lr.max() > 1e6 * bl.max()       # the force law feeds both back in
        else:
            run.run(20)
        out.append(_state(run, glob))
        ani.close()
    assert out[0] == out[1]


# ---- the refusals ---------------------------------------------------------------------------------------------------------
def test_where_it_raises(model_cache, monkeypatch):
    import torch
    from lammps_ani_amd import ani_hip, harness as hx, md
    path = model_cache(*nh.WATER_MODEL)
    s, m, _ = nh.water30(ROOT)
    run, ani, _ = _loop(path, True, vflag=True)
    with pytest.raises(RuntimeError, match="set_images"):
        run.set_recenter((0.5, 0.5, 0.5))
    run.set_npt(300.0)
    run.set_images()
    with pytest.raises(RuntimeError, match="barostat"):
        run.set_recenter((0.5, 0.5, 0.5))
    run.set_npt(None)
    run.set_recenter((0.5, 0.5, 0.5))
    with pytest.raises(RuntimeError, match="set_recenter"):
        run.set_npt(300.0)
    with pytest.raises(RuntimeError, match="recentring or an angular"):
        run.set_images(False)
    run.set_recenter(False)
    with pytest.raises(ValueError, match="three finite fractions"):
        run.set_recenter((0.5, 0.5))
    run.set_images(False)
    for call in (lambda: run.zero_momentum(angular=True), lambda: run.set_momentum(5, angular=True)):
        with pytest.raises(RuntimeError, match="set_images"):
            call()
    run.zero_momentum()                                                      # linear alone needs no image flags
    with pytest.raises(ValueError, match="every"):
        run.set_momentum(-1)
    with pytest.raises(ValueError, match="linear, angular"):
        run.set_momentum(5, linear=False)
    run.set_images()
    run.set_momentum(5, angular=True)
    with pytest.raises(RuntimeError, match="recentring or an angular"):
        run.set_images(False)
    run.set_momentum(0)
    run.set_images(False)
    monkeypatch.setattr(run.dc, "multi", True)                               # what a loop on two ranks, or force_collectives, sees
    for call in (run.com_state, run.zero_momentum, lambda: run.set_momentum(5),
                 lambda: run.set_recenter((0.5, 0.5, 0.5)), lambda: run.create_velocities(300.0, rot=True)):
        with pytest.raises(RuntimeError, match="one rank only"):
            call()
    ani.close()
    dev = torch.device("cuda:0")
    ani = ani_hip.ANI(path, 0, -1, use_single=True)
    with pytest.raises(ValueError, match="atom_masses must be 30"):
        md.VerletRun(ani, hx.decompose(s), s.boxhi - s.boxlo, dev, dt=DT, box_lo=s.boxlo, atom_masses=m[:29])
    with pytest.raises(RuntimeError, match="atom_masses: one rank only"):
        md.VerletRun(ani, hx.decompose(s), s.boxhi - s.boxlo, dev, dt=DT, box_lo=s.boxlo, atom_masses=m, force_collectives=True)
    monkeypatch.setenv("ANI_MD_NATIVE_REBUILD", "0")
    with pytest.raises(RuntimeError, match="atom_masses needs the device loop with native"):
        md.VerletRun(ani, hx.decompose(s), s.boxhi - s.boxlo, dev, dt=DT, box_lo=s.boxlo, atom_masses=m)
    run = md.VerletRun(ani, hx.decompose(s), s.boxhi - s.boxlo, dev, dt=DT, box_lo=s.boxlo)
    for call in (run.com_state, run.zero_momentum, lambda: run.set_momentum(5),
                 lambda: run.set_recenter((0.5, 0.5, 0.5))):
        with pytest.raises(RuntimeError, match="native re-neighbouring"):
            call()
    ani.close()
