"""What umbrella restraints cost in the timestep loop: ms per step of the same run with and without VerletRun.set_restraints on the
100 002-atom water box of the benchmark (ANI-2x shaped, 1 member), one rank, fp32 handle, ghost fold and native re-neighbouring as
bench.py runs it, dt 0.5 fs, velocities at 300 K.  Two torsions (PLUMED's KAPPA=100 kJ/mol/rad^2, centres 0.1 rad off the start) on
eight arbitrary atoms -- the two restraints of the alanine-dipeptide umbrella windows -- with a series row every 100 steps.  A
restrained step is the same step with two more launches behind the force evaluation (one thread per restraint; one thread per
touched atom plus the workgroup of the sums); the one-launch step boundary stays.
5 warm-up steps of each kind, then four rounds of 200 timed steps (`run(200)`) of each kind between two events on the stream; the
unthermostatted run heats up and re-neighbours more often as it goes, so the kind that goes first alternates from round to round
and the ratio is taken over the sums of all rounds; then the two launches alone, 200 each between two events.
usage: python tools/restraint_cost.py OUT.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; _pkg.load()
from lammps_ani_amd import ani_hip, harness as hx, md, model_file as mf

dev = torch.device("cuda:0")
N, STEPS, REPS, ROUNDS = 100002, 200, 200, 4
path = "/tmp/restraint_cost_ani2x.anim"
mf.write_model(path, mf.synthetic_model("ani2x", 1, seed=2024))
sysm = hx.spatial_sort(hx.water_box(N, seed=12345))
ani = ani_hip.ANI(path, 0)
run = md.VerletRun(ani, hx.decompose(sysm), sysm.boxhi - sysm.boxlo, dev, dt=0.5, box_lo=sysm.boxlo)
run.warm_paths()
run.create_velocities(300.0)
KAPPA = 23.9006
tags = [(1000, 1001, 1002, 1003), (50001, 50002, 50003, 50004)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b0 = run.nbuilds
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), run.nbuilds - b0


def restraints(on):
    if not on:
        run.set_restraints([])
        return
    run.set_restraints([("torsion", t, 0.0, 0.0) for t in tags])
    cv = run.restraint_state()["cv"]
    run.set_restraints([("torsion", t, KAPPA, float(c) + 0.1) for t, c in zip(tags, cv)], stride=100)


res = dict(natoms=N, ntotal=int(run.ntotal), npairs=int(run.npairs), members=1, dt_fs=0.5, restraints=2, kappa=KAPPA, stride=100,
           timed_steps=STEPS, extra_launches_per_step=2, plain_step_ms=[], plain_rebuilds=[], restrained_step_ms=[], restrained_rebuilds=[])
for on in (True, False):
    restraints(on)
    run.run(5)
for r in range(ROUNDS):
    order = ((False, "plain"), (True, "restrained"))
    for on, key in (order if r % 2 == 0 else order[::-1]):
        restraints(on)
        ms, nb = timed(lambda: run.run(STEPS))
        res[key + "_step_ms"].append(ms / STEPS)
        res[key + "_rebuilds"].append(nb)
        if on:
            st, ser = run.restraint_state(), run.restraint_series()
res["order"] = ["plain first" if r % 2 == 0 else "restrained first" for r in range(ROUNDS)]
res["restrained_over_plain"] = sum(res["restrained_step_ms"]) / sum(res["plain_step_ms"])
res["restrained_over_plain_by_round"] = [a / b for a, b in zip(res["restrained_step_ms"], res["plain_step_ms"])]
res["state_after"] = dict(evaluations=st["evaluations"], ebias=st["ebias"], nonfinite=st["nonfinite"], max_delta=st["max_delta"],
                          cv=st["cv"].tolist(), series_rows=int(ser["step"].shape[0]), series_last_step=int(ser["step"][-1]))

# the two launches alone
restraints(True)
rs, n, s, lib = run._restr, run.nlocal, run._stream, run._md
piece = {
    "eval": lambda: lib.ani_md_restraints_eval(run.x.data_ptr(), n, rs["atoms"].data_ptr(), rs["kind"].data_ptr(), rs["kappa"].data_ptr(),
                                               rs["centre"].data_ptr(), rs["nr"], run._len3.ctypes.data, None, run._pmask,
                                               rs["cv"].data_ptr(), rs["e"].data_ptr(), rs["fslot"].data_ptr(), rs["w"].data_ptr(), s),
    "apply": lambda: lib.ani_md_restraints_apply(run.f.data_ptr(), n, run.ev.data_ptr(), 0, rs["touched"].data_ptr(), rs["row_ptr"].data_ptr(),
                                                 rs["entries"].data_ptr(), rs["nt"], rs["fslot"].data_ptr(), rs["cv"].data_ptr(),
                                                 rs["e"].data_ptr(), rs["w"].data_ptr(), rs["centre"].data_ptr(), rs["kind"].data_ptr(),
                                                 rs["nr"], rs["rec"].data_ptr(), 0.0, None, s),
}
keep_f, keep_ev = run.f.clone(), run.ev.clone()
res["pieces_us"] = {}
for name, fn in piece.items():
    ms, _ = timed(lambda: [fn() for _ in range(REPS)])
    res["pieces_us"][name] = 1e3 * ms / REPS
    run.f.copy_(keep_f)
    run.ev.copy_(keep_ev)
out = {"command": "python tools/restraint_cost.py profiles/restraint_cost.json",
       "protocol": "5 warm-up steps of each kind, then run(200) without and with two torsion restraints between two events on the "
                   "stream, four rounds, the kind that goes first alternating; the ratio over the sums of the rounds; the two "
                   "launches alone as 200 launches each between two events",
       "water_100002_x1": res}
print(json.dumps(res), flush=True)
ani.close()
json.dump(out, open(sys.argv[1], "w"), indent=1)
