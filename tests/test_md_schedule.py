"""GPU: the schedule of the timestep loop (VerletRun.step / run / minimize) as the list of its ani_md_* launches,
and run(N) against N step() calls.

The reference's 30-atom water box of tests/test_nvt_md.py with its start velocities, fp32 handle only: the loop's own kernels are
fp64 whatever the handle, and nothing here depends on block or wave boundaries (the kernels have their own edge tests).

Launch traces.  `every` = 1, so that every step that does not rebuild has a look of the host in it.  Three step() calls, the middle
one with force_rebuild, then run(3) on the same loop, with the model as the calculator (its ghost exchanges are part of the trace).
The names are written without their ani_md_ prefix; the two integrators that take a step number carry it behind an @, and
nh_chain carries a * where it is given fresh partial sums.  The lists are those of the loop before it had a single schedule.

State.  run(7) against seven step() calls from the same start with the elementwise calculator of tests/test_shake_md.py (the
model's force kernels add in arrival order), `every` = 2: bitwise for the plain, Langevin and constrained loops, as the docstring of
run() promises; with a thermostat at the bar of tests/test_nvt_md.py (1e-12: every step() call begins with a fresh kinetic sum,
run() carries the one it scaled itself), the forces at that bar times the calculator's largest slope 30 * 2 pi / L.
"""
import os

import numpy as np
import pytest

import nh_reference as nh
import shake_reference as sr
from lammps_ani_amd import harness as hx
from test_shake_md import _Recorder, _periodic_forces

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.5

NOTES = {"ani_md_final_integrate": lambda a: f"@{a[9]}", "ani_md_final_initial_integrate": lambda a: f"@{a[11]}",
         "ani_md_nh_chain": lambda a: "*" if a[2] else ""}


class _Trace(_Recorder):
    """_Recorder that writes the step number behind the two integrators that take one, and a * behind a chain half-step that reads
    fresh partial sums"""

    def __getattr__(self, name):
        call = _Recorder.__getattr__(self, name)
        note = NOTES.get(name)
        if note is None:
            return call

        def noted(*args):
            rc = call(*args)
            self._calls[-1] += note(args)
            return rc
        return noted


def _loop(model_path, nvt=False, constrained=False, **kw):
    import torch
    from lammps_ani_amd import ani_hip, md
    s, _, v0 = nh.water30(ROOT)
    ani = ani_hip.ANI(model_path, 0, -1, use_single=True)
    run = md.VerletRun(ani, hx.decompose(s), s.boxhi - s.boxlo, torch.device("cuda:0"), dt=DT, box_lo=s.boxlo, **kw)
    tag = run.tag.cpu().numpy()
    run.v.copy_(torch.as_tensor(np.array(v0[tag])))
    if nvt:
        run.set_nvt(nh.T_TARGET, t_period=nh.T_PERIOD, mtchain=nh.MTCHAIN)
    if constrained:
        run.set_constraints(sr.water_oh_bonds(s), tol=1e-12)
        run.project_velocities()

    def to_global(t):
        out = np.zeros((s.natoms, 3))
        out[tag] = t[: run.nlocal].cpu().numpy()
        return out

    return run, ani, to_global, s


REBUILD = ["wrap_positions", "ghost_shell_count", "ghost_shell_fill", "append_ghosts", "check"]
NH_FIRST = ["nh_chain*", "nh_initial_integrate"]
NH_LAST = ["nh_chain*", "nh_scale"]
NHC_LAST = ["rattle_velocities", "nh_kinetic"] + NH_LAST

# configuration: (keywords of _loop, environment, trace of step() step(force_rebuild=True) step(), trace of run(3))
CONFIGS = {
    "plain": ({}, {},
              ["initial_integrate", "check", "final_integrate@1",
               "initial_integrate"] + REBUILD + ["final_integrate@2",
               "initial_integrate", "check", "final_integrate@3"],
              ["initial_integrate", "check", "final_initial_integrate@4", "check", "final_initial_integrate@5", "check",
               "final_integrate@6"]),
    "langevin": (dict(langevin=(300.0, 100.0)), {},
                 ["initial_integrate", "check", "final_integrate@1",
                  "initial_integrate"] + REBUILD + ["final_integrate@2",
                  "initial_integrate", "check", "final_integrate@3"],
                 ["initial_integrate", "check", "final_initial_integrate@4", "check", "final_initial_integrate@5", "check",
                  "final_integrate@6"]),
    "constrained": (dict(constrained=True), {},
                    ["initial_integrate", "shake_positions", "check", "final_integrate@1", "rattle_velocities",
                     "initial_integrate", "shake_positions"] + REBUILD + ["final_integrate@2", "rattle_velocities",
                     "initial_integrate", "shake_positions", "check", "final_integrate@3", "rattle_velocities"],
                    ["initial_integrate", "shake_positions", "check", "final_integrate@4", "rattle_velocities",
                     "initial_integrate", "shake_positions", "check", "final_integrate@5", "rattle_velocities",
                     "initial_integrate", "shake_positions", "check", "final_integrate@6", "rattle_velocities"]),
    "nvt": (dict(nvt=True), {},
            ["nh_kinetic"] + NH_FIRST + ["check", "nh_final_integrate"] + NH_LAST +
            ["nh_kinetic"] + NH_FIRST + REBUILD + ["nh_final_integrate"] + NH_LAST +
            ["nh_kinetic"] + NH_FIRST + ["check", "nh_final_integrate"] + NH_LAST,
            ["nh_kinetic"] + NH_FIRST + ["check", "nh_final_integrate"] + NH_LAST +
            ["nh_chain", "nh_initial_integrate", "check", "nh_final_integrate"] + NH_LAST +
            ["nh_chain", "nh_initial_integrate", "check", "nh_final_integrate"] + NH_LAST),
    "nvt_constrained": (dict(nvt=True, constrained=True), {},
                        ["nh_kinetic"] + NH_FIRST + ["shake_positions", "check", "final_integrate@1"] + NHC_LAST +
                        ["nh_kinetic"] + NH_FIRST + ["shake_positions"] + REBUILD + ["final_integrate@2"] + NHC_LAST +
                        ["nh_kinetic"] + NH_FIRST + ["shake_positions", "check", "final_integrate@3"] + NHC_LAST,
                        ["nh_kinetic"] + NH_FIRST + ["shake_positions", "check", "final_integrate@4"] + NHC_LAST +
                        ["nh_chain", "nh_initial_integrate", "shake_positions", "check", "final_integrate@5"] + NHC_LAST +
                        ["nh_chain", "nh_initial_integrate", "shake_positions", "check", "final_integrate@6"] + NHC_LAST),
    "overlap": (dict(overlap=True), {},
                ["initial_integrate", "check", "forward_ghosts", "reverse_ghosts", "final_integrate@1",
                 "initial_integrate"] + REBUILD + ["reverse_ghosts", "final_integrate@2",
                 "initial_integrate", "check", "forward_ghosts", "reverse_ghosts", "final_integrate@3"],
                ["initial_integrate", "check", "forward_ghosts", "reverse_ghosts", "final_initial_integrate@4",
                 "check", "forward_ghosts", "reverse_ghosts", "final_initial_integrate@5",
                 "check", "forward_ghosts", "reverse_ghosts", "final_integrate@6"]),
    "no_fold": ({}, {"ANI_MD_FOLD": "0"},
                ["initial_integrate", "check", "forward_ghosts", "reverse_ghosts", "final_integrate@1",
                 "initial_integrate"] + REBUILD + ["reverse_ghosts", "final_integrate@2",
                 "initial_integrate", "check", "forward_ghosts", "reverse_ghosts", "final_integrate@3"],
                ["initial_integrate", "check", "forward_ghosts", "reverse_ghosts", "final_initial_integrate@4",
                 "check", "forward_ghosts", "reverse_ghosts", "final_initial_integrate@5",
                 "check", "forward_ghosts", "reverse_ghosts", "final_integrate@6"]),
    # the tensor forms of re-neighbouring and of the look launch nothing of ani_md_*, and the ghost fold is on
    "tensor_rebuild": ({}, {"ANI_MD_NATIVE_REBUILD": "0"},
                       ["initial_integrate", "final_integrate@1", "initial_integrate", "final_integrate@2",
                        "initial_integrate", "final_integrate@3"],
                       ["initial_integrate", "final_initial_integrate@4", "final_initial_integrate@5", "final_integrate@6"]),
}
MINIMIZE = ["fire_work_size", "fire_init", "fire_iterate", "fire_iterate", "fire_check", "fire_iterate", "fire_iterate", "fire_check"]


def _names(calls):
    assert all(c.startswith("ani_md_") for c in calls)
    return [c[len("ani_md_"):] for c in calls]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_launch_traces_of_step_and_run(config, model_cache, monkeypatch):
    kw, env, want_steps, want_run = CONFIGS[config]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run, ani, _, _ = _loop(model_cache(*nh.WATER_MODEL), every=1, **kw)
    assert run._fold == (config not in ("overlap", "no_fold")) and run._native_rebuild == (config != "tensor_rebuild")
    calls = []
    run._md = _Trace(run._md, calls)
    builds0 = run.nbuilds
    for k in range(3):
        run.step(force_rebuild=(k == 1))
    got_steps = _names(calls)
    del calls[:]
    run.run(3)
    got_run = _names(calls)
    print(f"{config}: step x 3 {got_steps}\n{config}: run(3) {got_run}")
    assert run.nbuilds == builds0 + 1 and run.step_no == 6      # no look asked for a rebuild of its own
    assert got_steps == want_steps
    assert got_run == want_run
    if config == "plain":
        del calls[:]
        out = run.minimize(0.0, 0.0, 3, check_every=2)
        got_min = _names(calls)
        print(f"{config}: minimize {got_min}")
        assert out["iterations"] == 3 and out["stop"] == "maxiter" and out["rebuilds"] == 0
        assert got_min == MINIMIZE
    ani.close()


@pytest.mark.parametrize("config", ["plain", "langevin", "constrained", "nvt", "nvt_constrained"])
def test_run_and_steps_end_in_the_same_state(config, model_cache):
    kw = CONFIGS[config][0]
    out = []
    for stepwise in (False, True):
        run, ani, glob, s = _loop(model_cache(*nh.WATER_MODEL), every=2, **kw)
        _periodic_forces(run, s)
        x0 = glob(run.x)
        if stepwise:
            for _ in range(7):
                run.step()
        else:
            run.run(7)
        assert run.step_no == 7
        out.append((glob(run.x), glob(run.v), glob(run.f), x0))
        ani.close()
    (xa, va, fa, x0), (xb, vb, fb, _) = out
    print(f"{config}: run(7) against 7 step(): max |dx| {np.abs(xa - xb).max():.2e} |dv| {np.abs(va - vb).max():.2e} "
          f"|df| {np.abs(fa - fb).max():.2e}")
    assert np.abs(xa - x0).max() > 1e-3                           # the run moved
    if not kw.get("nvt"):
        assert xa.tobytes() == xb.tobytes() and va.tobytes() == vb.tobytes() and fa.tobytes() == fb.tobytes()
        return
    assert np.allclose(va, vb, rtol=1e-12, atol=1e-12 * np.abs(va).max()) and np.allclose(xa, xb, rtol=1e-12, atol=1e-12)
    slope = 30.0 * 2.0 * np.pi / (s.boxhi - s.boxlo).min()
    assert np.abs(fa - fb).max() <= slope * (1e-12 + 1e-12 * np.abs(xa).max())
