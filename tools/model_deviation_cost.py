"""What a model-deviation step costs (ani_request_model_deviation): unarmed, energy-only armed and force-armed steps through
ani_compute_full_device with the ghost fold installed, on the two eight-member BASELINE boxes.  Protocol of
profiles/atom_virial_notes.md: 5 warm-up and 40 timed steps per configuration, the three configurations alternating, each twice;
"step" is host wall time per call with one synchronisation after the 40 calls, "aev_bwd" the backward phase of ani_phase_times
(the step's own backward kernel; the deviation passes run after the phases).
usage: python tools/model_deviation_cost.py OUT.json"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import _pkg; _pkg.load()
from lammps_ani_amd import ani_hip, harness as hx, model_file as mf

dev = torch.device("cuda:0")
out = {}
cases = [("water_10002_x8", "ani2x", False, hx.spatial_sort(hx.water_box(10002, seed=12345))),
         ("ch4o2_100008_x8", "ani1x", True, hx.spatial_sort(hx.combustion_box(100008, seed=12345)))]
for name, kind, rep, sysm in cases:
    path = f"/tmp/mdc_{kind}.anim"
    mf.write_model(path, mf.synthetic_model(kind, 8, seed=2024, repulsion=rep))
    inp = hx.decompose(sysm)
    nt, nl = inp.ntotal, inp.nlocal
    d_x = torch.from_numpy(inp.x.reshape(-1).copy()).to(dev)
    d_sp = torch.from_numpy(inp.species.astype(np.int32)).to(dev)
    d_il = torch.from_numpy(inp.ilist).to(dev); d_nn = torch.from_numpy(inp.numneigh).to(dev); d_jl = torch.from_numpy(inp.jlist).to(dev)
    d_f = torch.zeros(nt * 3, dtype=torch.float64, device=dev); d_ev = torch.zeros(10, dtype=torch.float64, device=dev)
    owner = torch.from_numpy(np.asarray(inp.owner_lidx, dtype=np.int64)).to(dev)
    shift = torch.from_numpy((inp.x[nl:] - inp.x[np.asarray(inp.owner_lidx)]).reshape(-1).copy()).to(dev)
    M = 8
    bufs = dict(member_energy=torch.zeros(M, dtype=torch.float64, device=dev), atom_energy_dev=torch.zeros(nl, dtype=torch.float64, device=dev),
                member_dforce=torch.zeros(nt * M * 3, dtype=torch.float64, device=dev), atom_force_dev=torch.zeros(nl, dtype=torch.float64, device=dev),
                summary=torch.zeros(4, dtype=torch.float64, device=dev))
    energy_only = {k: bufs[k].data_ptr() for k in ("member_energy", "atom_energy_dev")}
    force = {k: v.data_ptr() for k, v in bufs.items()}
    st = torch.cuda.current_stream().cuda_stream
    ani = ani_hip.ANI(path, 0)
    ani.set_option("device_overwrite_forces", 1)
    ani.compute_device(nt, nl, d_sp.data_ptr(), d_x.data_ptr(), inp.npairs, d_il.data_ptr(), d_jl.data_ptr(), d_nn.data_ptr(), 0,
                       d_f.data_ptr(), d_ev.data_ptr(), stream=st)
    ani.set_ghost_fold(owner.data_ptr(), shift.data_ptr(), nt - nl)
    res = dict(ntotal=nt, nlocal=nl, npairs=int(inp.npairs), members=M, repulsion=rep)

    def run(cfg):
        arm = {"unarmed": None, "energy_only": energy_only, "force": force}[cfg]
        def step():
            ani.compute_device(nt, nl, 0, d_x.data_ptr(), inp.npairs, 0, 0, 0, 1, d_f.data_ptr(), d_ev.data_ptr(), vflag=True,
                               stream=st, d_deviation=arm)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        ani.phase_timing(1)
        t0 = time.perf_counter()
        for _ in range(40):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / 40 * 1e3
        ph = ani.phase_times()
        ani.phase_timing(0)
        c = max(ph["calls"], 1)
        return dict(step_ms_wall=ms, phases_ms={k: ph[k] / c for k in ("aev_fwd", "mlp", "aev_bwd", "other", "compact")}, calls=ph["calls"],
                    mlp_kernel=ani.last_mlp_kernel())

    for r in range(2):
        for cfg in ("unarmed", "energy_only", "force"):
            res[f"{cfg}_run{r}"] = run(cfg)
            print(name, cfg, r, json.dumps(res[f"{cfg}_run{r}"]), flush=True)
    torch.cuda.synchronize()
    s = bufs["summary"].cpu().numpy()
    res["last_summary"] = s.tolist()
    ani.close()
    out[name] = res
json.dump(out, open(sys.argv[1], "w"), indent=1)
