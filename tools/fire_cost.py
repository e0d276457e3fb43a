"""What one FIRE iteration of VerletRun.minimize costs beside one MD step of the same run, on the 100 002-atom water box of the
benchmark (ANI-2x shaped, 1 member), one rank, fp32 handle, ghost fold and native re-neighbouring as bench.py runs it.  An iteration
is the same force evaluation plus the three FIRE launches; both loops look at the host every 10 steps / iterations.
5 warm-up steps and a 5-iteration warm-up minimisation, then 50 timed MD steps (`run(50)`, NVE from rest) and a timed
minimisation of 50 iterations (etol = ftol = 0: 51 force evaluations, its set-up included) between two events on the stream, each
kind twice, alternating.  ms per step, ms per iteration (elapsed / 50) and per force evaluation (elapsed / 51).
usage: python tools/fire_cost.py OUT.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; _pkg.load()
from lammps_ani_amd import ani_hip, harness as hx, md, model_file as mf

dev = torch.device("cuda:0")
N, ITER = 100002, 50
path = "/tmp/fire_cost_ani2x.anim"
mf.write_model(path, mf.synthetic_model("ani2x", 1, seed=2024))
sysm = hx.spatial_sort(hx.water_box(N, seed=12345))
inp = hx.decompose(sysm)
ani = ani_hip.ANI(path, 0)
run = md.VerletRun(ani, inp, sysm.boxhi - sysm.boxlo, dev, dt=0.5, box_lo=sysm.boxlo)
run.warm_paths()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b0 = run.nbuilds
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), run.nbuilds - b0, r


run.run(5)
run.minimize(0.0, 0.0, 5)
res = dict(natoms=N, ntotal=int(run.ntotal), npairs=int(run.npairs), members=1, timed_steps=ITER, timed_iterations=ITER, step_ms=[],
           step_rebuilds=[], fire_iteration_ms=[], fire_per_force_evaluation_ms=[], fire_rebuilds=[], minimize=[])
for r in range(2):
    ms, nb, _ = timed(lambda: run.run(ITER))
    res["step_ms"].append(ms / ITER)
    res["step_rebuilds"].append(nb)
    ms, nb, out = timed(lambda: run.minimize(0.0, 0.0, ITER))
    res["fire_iteration_ms"].append(ms / ITER)
    res["fire_per_force_evaluation_ms"].append(ms / out["force_evaluations"])
    res["fire_rebuilds"].append(nb)
    res["minimize"].append(out)
res["fire_iteration_over_step"] = min(res["fire_iteration_ms"]) / min(res["step_ms"])
res["fire_evaluation_over_step"] = min(res["fire_per_force_evaluation_ms"]) / min(res["step_ms"])
out = {"command": "python tools/fire_cost.py profiles/fire_minimize_cost.json",
       "protocol": "5 warm-up steps and a 5-iteration minimisation, then run(50) and minimize(0, 0, 50) between two events on the stream, "
                   "each twice, alternating; ms per step / per iteration (elapsed / 50) / per force evaluation (elapsed / 51)",
       "water_100002_x1": res}
print(json.dumps(res), flush=True)
ani.close()
json.dump(out, open(sys.argv[1], "w"), indent=1)
