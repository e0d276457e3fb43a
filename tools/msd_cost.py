"""What image flags, MSD sampling and frame packing cost in the timestep loop: the 100 002-atom water box of the benchmark (ANI-2x
shaped, 1 member), one rank, fp32 handle, ghost fold and native re-neighbouring as bench.py runs it, dt 0.5 fs, 300 K.
Per call: 200 launches of ani_md_msd_sample (both of its launches) and of ani_md_frame_pack on fixed positions, each between its own
pair of events on the stream, after 20 warm calls; median, min, max and the 10th / 90th percentile -- for the group sets all, O, H
(one class each) and all + O + H together (two classes, three groups: what a water run asks for).
Per rebuild step: step(force_rebuild=True) between two events, 10 times with and 10 times without image flags, alternating.
Per MD step: run(50) between two events with an MSD row every step, every 10th step and without (image flags on in all three, so
the difference is the sampling alone), each twice, alternating, after 5 warm-up steps of each kind.
usage: python tools/msd_cost.py OUT.json"""
import json, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; _pkg.load()
from lammps_ani_amd import ani_hip, harness as hx, md, model_file as mf

dev = torch.device("cuda:0")
N, STEPS, REPS, WARM, REBUILDS = 100002, 50, 200, 20, 10
path = os.path.join(tempfile.mkdtemp(prefix="msd_cost_"), "ani2x.anim")
mf.write_model(path, mf.synthetic_model("ani2x", 1, seed=2024))
sysm = hx.spatial_sort(hx.water_box(N, seed=12345))
ani = ani_hip.ANI(path, 0)
run = md.VerletRun(ani, hx.decompose(sysm), sysm.boxhi - sysm.boxlo, dev, dt=0.5, box_lo=sysm.boxlo)
run.warm_paths()
run.create_velocities(300.0)
run.run(5)
res = dict(natoms=N, ntotal=int(run.ntotal), members=1, dt_fs=0.5, timed_steps=STEPS, launches=REPS)
GROUP_SETS = {"all": {"all": None}, "O": {"O": "O"}, "H": {"H": "H"}, "all_O_H": {"all": None, "O": "O", "H": "H"}}


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


res["msd_sample"] = {}
for name, groups in GROUP_SETS.items():
    run.set_msd(groups)
    res["msd_sample"][name] = dict(spread(lambda: run._msd_sample(None)), classes=run._msd["nclass"], groups=len(groups))
run.set_msd({})
for unwrap in (False, True):
    run.set_dump(1, unwrap=unwrap, capacity=4)
    dp = run._dump

    def pack():
        dp["nring"], dp["steps"] = 0, []          # the same slot every time: no drain inside the timed region
        run._dump_frame()
    res["frame_pack_unwrapped" if unwrap else "frame_pack_wrapped"] = spread(pack)
    dp["nring"], dp["steps"] = 0, []
    run.set_dump(0)

res["rebuild_step_ms"] = dict(images=[], plain=[])
for r in range(REBUILDS):
    for name, on in (("plain", False), ("images", True)):
        run.set_images(on)
        res["rebuild_step_ms"][name].append(timed(lambda: run.step(force_rebuild=True), 1)[0])
res["rebuild_step_images_over_plain"] = float(np.median(res["rebuild_step_ms"]["images"]) / np.median(res["rebuild_step_ms"]["plain"]))

kinds = (("unsampled", 0), ("every_1", 1), ("every_10", 10))
run.set_images(True)


def arm(stride):
    run.set_msd(GROUP_SETS["all_O_H"] if stride else {}, stride=stride)


for name, stride in kinds:
    res[name + "_step_ms"], res[name + "_rebuilds"] = [], []
    arm(stride)
    run.run(5)
for r in range(2):
    for name, stride in kinds:
        arm(stride)
        ms, nb = timed(lambda: run.run(STEPS), STEPS)
        res[name + "_step_ms"].append(ms)
        res[name + "_rebuilds"].append(nb)
base = min(res["unsampled_step_ms"])
res["every_1_over_unsampled"] = min(res["every_1_step_ms"]) / base
res["every_10_over_unsampled"] = min(res["every_10_step_ms"]) / base
res["sample_over_unsampled_step"] = res["msd_sample"]["all_O_H"]["median_us"] / 1000.0 / base
out = {"command": "python tools/msd_cost.py profiles/msd_cost.json",
       "protocol": "per call: 20 warm calls, then 200 calls each between its own two events on the stream (median, spread); per rebuild "
                   "step: step(force_rebuild=True) between two events, 10 with and 10 without image flags, alternating; per step: 5 "
                   "warm-up steps of each kind, then run(50) between two events with an MSD row (all, O, H) every step, every 10th and "
                   "without, image flags on throughout, each twice, alternating",
       "water_100002_x1": res}
print(json.dumps(res), flush=True)
ani.close()
json.dump(out, open(sys.argv[1], "w"), indent=1)
