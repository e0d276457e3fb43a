"""What the Nose-Hoover chain costs in the timestep loop: ms per step of the same run with and without VerletRun.set_nvt on the
100 002-atom water box of the benchmark (ANI-2x shaped, 1 member), one rank, fp32 handle, ghost fold and native re-neighbouring as
bench.py runs it, dt 0.5 fs, velocities at 300 K, target 300 K, t_period 50 fs, three links.  A thermostatted step is the same force
evaluation with five launches at its boundary (chain, scaled initial integrate, final integrate with the partial sums, chain,
scale) where the plain run has one (final + initial fused); with all 66 668 O-H bonds constrained it is eight (chain, scaled
initial, position stage, final, velocity stage, kinetic, chain, scale) against the constrained run's four.
5 warm-up steps of each kind, then 50 timed steps (`run(50)`) between two events on the stream, each kind twice, alternating; then
the pieces alone, 200 launches each between two events; then one thermo() record (its two launches and the read).
usage: python tools/nvt_cost.py OUT.json"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; _pkg.load()
from lammps_ani_amd import ani_hip, harness as hx, md, model_file as mf

dev = torch.device("cuda:0")
N, STEPS, REPS = 100002, 50, 200
path = "/tmp/nvt_cost_ani2x.anim"
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
ani = ani_hip.ANI(path, 0)
run = md.VerletRun(ani, hx.decompose(sysm), sysm.boxhi - sysm.boxlo, dev, dt=0.5, box_lo=sysm.boxlo)
run.warm_paths()
run.create_velocities(300.0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b0 = run.nbuilds
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), run.nbuilds - b0


def thermostat(on):
    run.set_nvt(300.0 if on else None, t_period=50.0)


res = dict(natoms=N, ntotal=int(run.ntotal), npairs=int(run.npairs), members=1, dt_fs=0.5, t_target=300.0, t_period_fs=50.0, mtchain=3,
           timed_steps=STEPS, launches_per_step=dict(plain_run=1, nvt=5, constrained=4, constrained_nvt=8),
           plain_step_ms=[], plain_rebuilds=[], nvt_step_ms=[], nvt_rebuilds=[], constrained_step_ms=[], constrained_nvt_step_ms=[])
for on in (True, False):
    thermostat(on)
    run.run(5)
for r in range(2):
    for on, key in ((False, "plain"), (True, "nvt")):
        thermostat(on)
        ms, nb = timed(lambda: run.run(STEPS))
        res[key + "_step_ms"].append(ms / STEPS)
        res[key + "_rebuilds"].append(nb)
res["nvt_over_plain"] = min(res["nvt_step_ms"]) / min(res["plain_step_ms"])
res["state_after"] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in run.nvt_state().items()}

# the pieces alone
n, st, lib = run.nlocal, run._stream, run._md
nvt = run._nvt
piece = {
    "kinetic": lambda: lib.ani_md_nh_kinetic(run.v.data_ptr(), nvt["mass"].data_ptr(), n, nvt["work"].data_ptr(), st),
    "chain_from_partials": lambda: lib.ani_md_nh_chain(nvt["state"].data_ptr(), nvt["work"].data_ptr(), nvt["npart"], 300.0,
                                                       3.0 * n - 3.0, nvt["par"], st),
    "chain_from_state": lambda: lib.ani_md_nh_chain(nvt["state"].data_ptr(), nvt["work"].data_ptr(), 0, 300.0, 3.0 * n - 3.0,
                                                    nvt["par"], st),
    "scale": lambda: lib.ani_md_nh_scale(run.v.data_ptr(), n, nvt["state"].data_ptr(), st),
}
keep_v, keep_state = run.v.clone(), nvt["state"].clone()
res["pieces_us"] = {}
for name, fn in piece.items():
    ms, _ = timed(lambda: [fn() for _ in range(REPS)])
    res["pieces_us"][name] = 1e3 * ms / REPS
    run.v.copy_(keep_v)
    nvt["state"].copy_(keep_state)
run.thermo()
t0 = time.perf_counter()
for _ in range(20):
    th = run.thermo()
res["thermo_call_us_wall"] = 1e6 * (time.perf_counter() - t0) / 20
res["thermo"] = {k: (None if v != v else v) for k, v in th.items()}   # no vflag in this run: the pressure entries are NaN

# with all O-H bonds constrained: the unfused boundary on both sides of the comparison
thermostat(False)
run.set_constraints(bonds, tol=1e-4, maxiter=20)
run.create_velocities(300.0)
run.run(5)
thermostat(True)
run.run(5)
for r in range(2):
    for on, key in ((False, "constrained"), (True, "constrained_nvt")):
        thermostat(on)
        ms, nb = timed(lambda: run.run(STEPS))
        res[key + "_step_ms"].append(ms / STEPS)
res["constrained_nvt_over_constrained"] = min(res["constrained_nvt_step_ms"]) / min(res["constrained_step_ms"])
res["constraint_stats"] = run.constraint_stats()
out = {"command": "python tools/nvt_cost.py profiles/nvt_cost.json",
       "protocol": "5 warm-up steps of each kind, then run(50) without and with the Nose-Hoover chain between two events on the "
                   "stream, each twice, alternating; the pieces alone as 200 launches between two events; the same pair of runs "
                   "with all O-H bonds constrained",
       "water_100002_x1": res}
print(json.dumps(res), flush=True)
ani.close()
json.dump(out, open(sys.argv[1], "w"), indent=1)
