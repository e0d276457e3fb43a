"""What the centre-of-mass sample, the momentum fix and recentring cost in the timestep loop: the 100 002-atom water box of the
benchmark (ANI-2x shaped, 1 member), one rank, fp32 handle, ghost fold and native re-neighbouring as bench.py runs it, dt 0.5 fs, a
loop made with langevin=(300, 100).
Per call: 200 launches of ani_md_com_sample (its two launches) on the loop's own arrays and of ani_md_com_apply on copies of them (so
that the trajectory stays), each between its own pair of events on the stream, after 20 warm calls; median, min, max and the 10th /
90th percentile.
Per MD step: run(50) between two events for the loop as it is (the base), with recentring every step and with fix momentum (linear
and angular) every 10th step -- each twice, alternating, after 5 warm-up steps of each kind.
usage: python tools/protocol_cost.py OUT.json"""
import json, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; _pkg.load()
from lammps_ani_amd import ani_hip, harness as hx, md, model_file as mf

dev = torch.device("cuda:0")
N, STEPS, REPS, WARM, DAMP = 100002, 50, 200, 20, 100.0
path = os.path.join(tempfile.mkdtemp(prefix="protocol_cost_"), "ani2x.anim")
mf.write_model(path, mf.synthetic_model("ani2x", 1, seed=2024))
sysm = hx.spatial_sort(hx.water_box(N, seed=12345))
ani = ani_hip.ANI(path, 0)
run = md.VerletRun(ani, hx.decompose(sysm), sysm.boxhi - sysm.boxlo, dev, dt=0.5, box_lo=sysm.boxlo, langevin=(300.0, DAMP))
run.warm_paths()
run.create_velocities(300.0)
run.set_images()
run.run(5)
res = dict(natoms=N, ntotal=int(run.ntotal), members=1, dt_fs=0.5, timed_steps=STEPS, launches=REPS, damp_fs=DAMP)


def spread(call):
    for _ in range(WARM):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in ev:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    t = 1000.0 * np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    return dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), p10_us=float(np.percentile(t, 10)),
                p90_us=float(np.percentile(t, 90)))


def timed(call, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b0 = run.nbuilds
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / count, run.nbuilds - b0


# ---- per call, on copies ------------------------------------------------------------------------------------------------------
lib, n, st = run._md, run.nlocal, run._stream
x, v, xb = (t[:n].clone() for t in (run.x, run.v, run.x_built))
d2 = torch.zeros(1, dtype=torch.float64, device=dev)
c = run._com_buffers()
res["com_sample"] = spread(run._com_sample)
for name, flags in (("com_apply_linear", 1), ("com_apply_linear_angular", 3), ("com_apply_recenter", 4)):
    # the record of the loop's own state, applied to the copies: the recentre bit gets a target that is the centre of mass itself
    run._com_sample()
    torch.cuda.synchronize()
    target = c["rec"][1:4].cpu().numpy().copy()
    res[name] = spread(lambda: lib.ani_md_com_apply(x.data_ptr(), v.data_ptr(), run._img.data_ptr(), n, c["rec"].data_ptr(), flags,
                                                    target.ctypes.data, 7, run._len3.ctypes.data, None, run._pmask, xb.data_ptr(),
                                                    d2.data_ptr(), st))
    x.copy_(run.x[:n])
    v.copy_(run.v)

# ---- per step ---------------------------------------------------------------------------------------------------------------
def arm(kind):
    run.set_recenter((0.5, 0.5, 0.5) if kind == "recenter" else None)
    run.set_momentum(10 if kind == "momentum_10" else 0, linear=True, angular=True)


kinds = ("plain", "recenter", "momentum_10")
for kind in kinds:
    res[kind + "_step_ms"], res[kind + "_rebuilds"] = [], []
    arm(kind)
    run.run(5)
for r in range(2):
    for kind in kinds:
        arm(kind)
        ms, nb = timed(lambda: run.run(STEPS), STEPS)
        res[kind + "_step_ms"].append(ms)
        res[kind + "_rebuilds"].append(nb)
base = min(res["plain_step_ms"])
for kind in kinds[1:]:
    res[kind + "_over_plain"] = min(res[kind + "_step_ms"]) / base
out = {"command": "python tools/protocol_cost.py profiles/protocol_cost.json",
       "protocol": "per call: 20 warm calls, then 200 calls each between its own two events on the stream (median, spread), on copies of "
                   "the loop's arrays; per step: 5 warm-up steps of each kind, then run(50) between two events, each kind twice, "
                   "alternating; the base is the same loop (langevin=(300, 100)) without a fix, in the same session",
       "water_100002_x1": res}
print(json.dumps(res), flush=True)
ani.close()
json.dump(out, open(sys.argv[1], "w"), indent=1)
