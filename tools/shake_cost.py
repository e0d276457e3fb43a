"""What bond constraints cost in the timestep loop: ms per step of the same run with and without VerletRun.set_constraints on the
100 002-atom water box of the benchmark (ANI-2x shaped, 1 member), one rank, fp32 handle, ghost fold and native re-neighbouring as
bench.py runs it, dt 0.5 fs, all 66 668 O-H bonds held at their current lengths (33 334 clusters of three atoms, tol 1e-4 and
20 iterations as `fix shake 0.0001 20`).  Velocities at 300 K, projected.  A constrained step is the same force evaluation with four
launches at its boundary (final, velocity stage, initial, position stage) where the plain run has one (final + initial fused).
5 warm-up steps of each kind, then 50 timed steps (`run(50)`) between two events on the stream, each kind twice, alternating; then
the two stages alone, 200 launches each between two events (the position stage on the positions as they are: no iteration, the
fixed cost of the launch and its loads; and from a free move of one step, restored before every launch, with the restoring copies
timed separately and subtracted).
usage: python tools/shake_cost.py OUT.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; _pkg.load()
from lammps_ani_amd import ani_hip, harness as hx, md, model_file as mf

dev = torch.device("cuda:0")
N, STEPS, REPS = 100002, 50, 200
path = "/tmp/shake_cost_ani2x.anim"
mf.write_model(path, mf.synthetic_model("ani2x", 1, seed=2024))
sysm = hx.spatial_sort(hx.water_box(N, seed=12345))


def oh_bonds(s):
    """every hydrogen with its nearest oxygen (minimum image): [nb, 2] global indices"""
    from scipy.spatial import cKDTree
    L = s.boxhi - s.boxlo
    xw = np.mod(s.x - s.boxlo, L)
    xw[xw >= L] = 0.0
    io, ih = np.nonzero(s.types == 4)[0], np.nonzero(s.types == 1)[0]
    dist, j = cKDTree(xw[io], boxsize=L).query(xw[ih])
    assert (dist < 1.3).all()
    return np.stack([io[j], ih], 1)


bonds = oh_bonds(sysm)
inp = hx.decompose(sysm)
ani = ani_hip.ANI(path, 0)
run = md.VerletRun(ani, inp, sysm.boxhi - sysm.boxlo, dev, dt=0.5, box_lo=sysm.boxlo)
run.warm_paths()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b0 = run.nbuilds
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), run.nbuilds - b0


def constrain(on):
    run.set_constraints(bonds if on else [], tol=1e-4, maxiter=20)


constrain(True)
run.create_velocities(300.0)
res = dict(natoms=N, ntotal=int(run.ntotal), npairs=int(run.npairs), members=1, bonds=int(len(bonds)), clusters=int(run._cons["nc"]),
           tol=1e-4, maxiter=20, dt_fs=0.5, timed_steps=STEPS, plain_step_ms=[], plain_rebuilds=[], constrained_step_ms=[],
           constrained_rebuilds=[], stats=[])
run.run(5)
constrain(False)
run.run(5)
for r in range(2):
    constrain(False)
    ms, nb = timed(lambda: run.run(STEPS))
    res["plain_step_ms"].append(ms / STEPS)
    res["plain_rebuilds"].append(nb)
    constrain(True)
    ms, nb = timed(lambda: run.run(STEPS))
    res["constrained_step_ms"].append(ms / STEPS)
    res["constrained_rebuilds"].append(nb)
    res["stats"].append(run.constraint_stats())
res["constrained_over_plain"] = min(res["constrained_step_ms"]) / min(res["plain_step_ms"])

# the two stages alone
n = run.nlocal
ms, _ = timed(lambda: [run.project_velocities() for _ in range(REPS)])
res["velocity_stage_us"] = 1e3 * ms / REPS
ms, _ = timed(lambda: [run._shake_positions() for _ in range(REPS)])
res["position_stage_converged_start_us"] = 1e3 * ms / REPS
x_keep, v_keep = run.x[:n].clone(), run.v.clone()
x_free = x_keep + run.dt * v_keep                      # a free move of one step from the constrained positions


def restore():
    run.x[:n].copy_(x_free)
    run.v.copy_(v_keep)


def moves():
    for _ in range(REPS):
        restore()
        run._shake_positions()


ms_all, _ = timed(moves)
ms_copy, _ = timed(lambda: [restore() for _ in range(REPS)])
res["position_stage_free_move_us"] = 1e3 * (ms_all - ms_copy) / REPS
res["position_stage_free_move_stats"] = run.constraint_stats()
run.x[:n].copy_(x_keep)
run.v.copy_(v_keep)
out = {"command": "python tools/shake_cost.py profiles/shake_cost.json",
       "protocol": "5 warm-up steps of each kind, then run(50) without and with all O-H bonds constrained between two events on the "
                   "stream, each twice, alternating; then 200 launches of each stage alone between two events",
       "water_100002_x1": res}
print(json.dumps(res), flush=True)
ani.close()
json.dump(out, open(sys.argv[1], "w"), indent=1)
