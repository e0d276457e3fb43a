"""What RDF sampling costs in the timestep loop: the 100 002-atom water box of the benchmark (ANI-2x shaped, 1 member), one rank,
fp32 handle, ghost fold and native re-neighbouring as bench.py runs it, dt 0.5 fs, 300 K.  O-O, O-H, H-O, H-H with 200 bins to 5.1 A.
Per sample: 200 back-to-back ani_rdf_accumulate_device launches on fixed positions, each between its own pair of events on the
stream, after 20 warm launches; median, min, max and the 10th / 90th percentile, for every kernel shape (16 lanes or a wave per
centre, LDS histogram or global atomics).  Per MD step: run(50) between two events with sampling every step, every 10th step and
without, each twice, alternating, after 5 warm-up steps of each kind.
usage: python tools/rdf_cost.py OUT.json [NOTES.md]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; _pkg.load()
from lammps_ani_amd import ani_hip, harness as hx, md, model_file as mf

dev = torch.device("cuda:0")
N, STEPS, REPS, WARM = 100002, 50, 200, 20
PAIRS, NBINS, RMAX = [("O", "O"), ("O", "H"), ("H", "O"), ("H", "H")], 200, 5.1
path = "/tmp/rdf_cost_ani2x.anim"
mf.write_model(path, mf.synthetic_model("ani2x", 1, seed=2024))
sysm = hx.spatial_sort(hx.water_box(N, seed=12345))
inp = hx.decompose(sysm)
ani = ani_hip.ANI(path, 0)
run = md.VerletRun(ani, inp, sysm.boxhi - sysm.boxlo, dev, dt=0.5, box_lo=sysm.boxlo)
run.warm_paths()
run.create_velocities(300.0)
res = dict(natoms=N, ntotal=int(run.ntotal), npairs=int(run.npairs), members=1, pairs=["-".join(p) for p in PAIRS], nbins=NBINS,
           rmax=RMAX, dt_fs=0.5, timed_steps=STEPS, sample_launches=REPS)


def sample_times(lanes, lds):
    """ms of each of REPS launches between its own events, on the loop's positions as they are"""
    ani.set_option("rdf_lanes", lanes)
    ani.set_option("rdf_lds", lds)
    run.rdf(reset=True)
    for _ in range(WARM):
        run.sample_rdf()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    x, nt, nl, st = run.x.data_ptr(), run.ntotal, run.nlocal, run._stream
    for e0, e1 in ev:
        e0.record()
        ani.rdf_accumulate_device(nt, nl, x, stream=st)
        e1.record()
    torch.cuda.synchronize()
    t = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        ani.rdf_accumulate_device(nt, nl, x, stream=st)
    e1.record()
    torch.cuda.synchronize()
    out = run.rdf(reset=True)
    assert out["frames"] == WARM + 2 * REPS
    return dict(lanes=lanes, lds=lds, median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()),
                p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)), back_to_back_ms=e0.elapsed_time(e1) / REPS,
                counted_per_frame=int(out["counts"].sum()) // out["frames"])


def timed_run():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b0 = run.nbuilds
    e0.record()
    run.run(STEPS)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS, run.nbuilds - b0


run.set_rdf(PAIRS, nbins=NBINS, rmax=RMAX, every=1)
run.run(5)
shapes = [sample_times(lanes, lds) for lanes, lds in ((16, 1), (64, 1), (16, 0), (64, 0))]
res["sample_shapes"] = shapes
best = min(shapes, key=lambda s: s["median_ms"])
res["default_shape"] = dict(lanes=16, lds=1)
res["fastest_shape"] = dict(lanes=best["lanes"], lds=best["lds"])
ani.set_option("rdf_lanes", 16)
ani.set_option("rdf_lds", 1)
res["sample_ms"] = shapes[0]["median_ms"]

kinds = (("unsampled", 0), ("every_1", 1), ("every_10", 10))
for name, every in kinds:
    res[name + "_step_ms"], res[name + "_rebuilds"] = [], []
for name, every in kinds:          # warm-up of each kind
    run.set_rdf(PAIRS if every else [], nbins=NBINS, rmax=RMAX, every=max(every, 1))
    run.run(5)
for r in range(2):
    for name, every in kinds:
        run.set_rdf(PAIRS if every else [], nbins=NBINS, rmax=RMAX, every=max(every, 1))
        ms, nb = timed_run()
        res[name + "_step_ms"].append(ms)
        res[name + "_rebuilds"].append(nb)
base = min(res["unsampled_step_ms"])
res["every_1_over_unsampled"] = min(res["every_1_step_ms"]) / base
res["every_10_over_unsampled"] = min(res["every_10_step_ms"]) / base
res["sample_over_unsampled_step"] = res["sample_ms"] / base
fm = os.path.join(ROOT, "profiles", "find_molecules_cost.json")
if os.path.exists(fm):
    ref = min(json.load(open(fm))["water_100002_x1"]["find_molecules_ms"])
    res["find_molecules_ms_recorded"] = ref
    res["sample_over_find_molecules"] = res["sample_ms"] / ref
out = {"command": "python tools/rdf_cost.py profiles/rdf_cost.json profiles/rdf_notes.md",
       "protocol": "per sample: 20 warm launches, then 200 launches each between its own two events on the stream (median, spread), and "
                   "200 back to back between one pair; per step: 5 warm-up steps of each kind, then run(50) between two events without "
                   "sampling, with every=1 and every=10, each twice, alternating",
       "water_100002_x1": res}
print(json.dumps(res), flush=True)
ani.close()
json.dump(out, open(sys.argv[1], "w"), indent=1)
if len(sys.argv) > 2:
    s0 = shapes[0]
    lines = ["# RDF sampling: cost on the 100 002-atom water box (tools/rdf_cost.py, profiles/rdf_cost.json)", "",
             f"O-O, O-H, H-O, H-H, {NBINS} bins to {RMAX} A; {s0['counted_per_frame']} entries counted per frame out of {res['npairs']} list entries.", "",
             "| lanes per centre | histogram | median ms | p10 | p90 | min | max | back to back |", "|---|---|---|---|---|---|---|---|"]
    for s in shapes:
        lines.append(f"| {s['lanes']} | {'LDS' if s['lds'] else 'global'} | {s['median_ms']:.4f} | {s['p10_ms']:.4f} | {s['p90_ms']:.4f} | "
                     f"{s['min_ms']:.4f} | {s['max_ms']:.4f} | {s['back_to_back_ms']:.4f} |")
    ms2 = lambda k: " / ".join(f"{v:.4f}" for v in res[k]) + f" (rebuilds {res[k.replace('_step_ms', '_rebuilds')]})"
    lines += ["", f"MD step of the same run, ms (two runs of {STEPS} steps each): unsampled {ms2('unsampled_step_ms')}, every=1 {ms2('every_1_step_ms')}, "
              f"every=10 {ms2('every_10_step_ms')}.",
              f"Ratios (best of each): every=1 {res['every_1_over_unsampled']:.3f}, every=10 {res['every_10_over_unsampled']:.3f} of an unsampled step; "
              f"one sample (16 lanes, LDS) is {res['sample_over_unsampled_step']:.3f} of an unsampled step"
              + (f" and {res['sample_over_find_molecules']:.3f} of the molecule finder's recorded {res['find_molecules_ms_recorded']:.3f} ms." if "sample_over_find_molecules" in res else "."),
              "The shipped shape is 16 lanes per centre with the LDS histogram; the other rows are the measurement options rdf_lanes / rdf_lds.", ""]
    open(sys.argv[2], "w").write("\n".join(lines))
