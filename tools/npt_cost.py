"""What the isotropic barostat costs in the timestep loop: ms per step of four kinds of run from one process on the 100 002-atom
water box of the benchmark (ANI-2x shaped, 1 member), one rank, fp32 handle, ghost fold and native re-neighbouring as bench.py runs it,
dt 0.5 fs, velocities at 300 K:
  nve          the plain loop of bench.py (no virial)
  nve_vflag    the same with the pair virial accumulated in every force evaluation
  nvt_vflag    set_nvt(300 K, t_period 50 fs, three links) on the loop with the virial
  npt          set_npt(300 K, 50 fs, p_start = the pressure of the start, p_period 500 fs, three links each) on that loop
nve_vflag / nve is what a per-step virial costs, npt / nvt_vflag what the barostat itself costs (the same five launches at the step's
boundary; the barostat's are a longer chain kernel, a first half that dilates and scales the ghost shifts, a second half that also
scales, and a look that carries the record and refreshes the host's box).  The target is the start's own pressure, so that the box
breathes without running away during the timing.
5 warm-up steps of each kind, then 50 timed steps (`run(50)`) between two events on the stream, each kind three times, alternating.
Two loops (with and without vflag) live side by side in the process; the barostat's box is carried across its repetitions.
usage: python tools/npt_cost.py OUT.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; _pkg.load()
from lammps_ani_amd import ani_hip, harness as hx, md, model_file as mf

dev = torch.device("cuda:0")
N, STEPS, ROUNDS = 100002, 50, 3
path = "/tmp/npt_cost_ani2x.anim"
mf.write_model(path, mf.synthetic_model("ani2x", 1, seed=2024))
sysm = hx.spatial_sort(hx.water_box(N, seed=12345))


def loop(vflag):
    ani = ani_hip.ANI(path, 0)
    run = md.VerletRun(ani, hx.decompose(sysm), sysm.boxhi - sysm.boxlo, dev, dt=0.5, box_lo=sysm.boxlo, vflag=vflag)
    run.warm_paths()
    run.create_velocities(300.0)
    return ani, run


def timed(run, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b0 = run.nbuilds
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), run.nbuilds - b0


ani0, plain = loop(False)
ani1, vrun = loop(True)
p0 = vrun.thermo()["press"]
kinds = {
    "nve": (plain, lambda: None),
    "nve_vflag": (vrun, lambda: vrun.set_npt(None)),
    "nvt_vflag": (vrun, lambda: vrun.set_nvt(300.0, t_period=50.0)),
    "npt": (vrun, lambda: vrun.set_npt(300.0, t_period=50.0, p_start=p0, p_period=500.0)),
}
res = dict(natoms=N, ntotal=int(vrun.ntotal), npairs=int(vrun.npairs), members=1, dt_fs=0.5, t_target=300.0, t_period_fs=50.0,
           p_target_atm=p0, p_period_fs=500.0, mtchain=3, mpchain=3, timed_steps=STEPS,
           launches_per_step=dict(nve=1, nve_vflag=1, nvt_vflag=5, npt=5), step_ms={k: [] for k in kinds}, rebuilds={k: [] for k in kinds})
for key, (run, setup) in kinds.items():
    setup()
    run.run(5)
for r in range(ROUNDS):
    for key, (run, setup) in kinds.items():
        setup()
        ms, nb = timed(run, lambda: run.run(STEPS))
        res["step_ms"][key].append(ms / STEPS)
        res["rebuilds"][key].append(nb)
        if key == "npt":
            st = run.npt_state()
            res.setdefault("npt_volume_ratio", []).append(st["vol"] / st["v0"])
            res["npt_thermo"] = {k: (None if v != v else v) for k, v in run.thermo().items()}
best = {k: min(v) for k, v in res["step_ms"].items()}
res["best_step_ms"] = best
res["virial_cost_nve_vflag_over_nve"] = best["nve_vflag"] / best["nve"]
res["nvt_vflag_over_nve_vflag"] = best["nvt_vflag"] / best["nve_vflag"]
res["barostat_cost_npt_over_nvt_vflag"] = best["npt"] / best["nvt_vflag"]
res["spread"] = {k: (max(v) - min(v)) / min(v) for k, v in res["step_ms"].items()}
out = {"command": "python tools/npt_cost.py profiles/npt_cost.json",
       "protocol": "two loops in one process (without and with vflag); 5 warm-up steps of each kind, then run(50) of each kind between "
                   "two events on the stream, three rounds, alternating; the smallest of the three is compared",
       "water_100002_x1": res}
print(json.dumps(res), flush=True)
ani0.close()
ani1.close()
json.dump(out, open(sys.argv[1], "w"), indent=1)
