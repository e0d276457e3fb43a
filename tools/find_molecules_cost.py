"""What one ani_find_molecules_device call costs beside a step of the same run, on the two 100 000-atom boxes of the benchmark:
the CH4/O2 gas (ANI-1x shaped, 8 members, repulsion; ~26 list entries per atom) and the water box (ANI-2x shaped, 1 member; ~150).
Both through ani_compute_full_device with the ghost fold installed, the finder with the owners of that fold.  5 warm-up calls, then
50 timed steps / 500 timed finder calls between two events on the stream, each kind twice, alternating.  The bond table is the analysis table of
tests/golden/bond_table_analysis.json.
usage: python tools/find_molecules_cost.py OUT.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; _pkg.load()
from lammps_ani_amd import ani_hip, harness as hx, model_file as mf

dev = torch.device("cuda:0")
fx = json.load(open(os.path.join(ROOT, "tests", "golden", "bond_table_analysis.json")))
out = {"command": "python tools/find_molecules_cost.py profiles/find_molecules_cost.json",
       "protocol": "5 warm-up, then 50 timed steps / 500 timed finder calls between two events on the stream, each kind twice, alternating; ms per call"}
cases = [("ch4o2_100008_x8", "ani1x", 8, True, hx.spatial_sort(hx.combustion_box(100008, seed=12345))),
         ("water_100002_x1", "ani2x", 1, False, hx.spatial_sort(hx.water_box(100002, seed=12345)))]
for name, kind, M, rep, sysm in cases:
    path = f"/tmp/fmc_{kind}.anim"
    mf.write_model(path, mf.synthetic_model(kind, M, seed=2024, repulsion=rep))
    inp = hx.decompose(sysm)
    nt, nl = inp.ntotal, inp.nlocal
    d_x = torch.from_numpy(inp.x.reshape(-1).copy()).to(dev)
    d_sp = torch.from_numpy(inp.species.astype(np.int32)).to(dev)
    d_il = torch.from_numpy(inp.ilist).to(dev); d_nn = torch.from_numpy(inp.numneigh).to(dev); d_jl = torch.from_numpy(inp.jlist).to(dev)
    d_f = torch.zeros(nt * 3, dtype=torch.float64, device=dev); d_ev = torch.zeros(10, dtype=torch.float64, device=dev)
    owner = torch.from_numpy(np.asarray(inp.owner_lidx, dtype=np.int64)).to(dev)
    shift = torch.from_numpy((inp.x[nl:] - inp.x[np.asarray(inp.owner_lidx)]).reshape(-1).copy()).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    ani = ani_hip.ANI(path, 0)
    sym = ani.species_symbols()
    ani.set_bond_table({(p[0], p[1]): v + fx["stretch_margin"] for p, v in fx["bond_lengths"].items() if p[0] in sym and p[1] in sym})
    ani.set_option("device_overwrite_forces", 1)
    ani.compute_device(nt, nl, d_sp.data_ptr(), d_x.data_ptr(), inp.npairs, d_il.data_ptr(), d_jl.data_ptr(), d_nn.data_ptr(), 0,
                       d_f.data_ptr(), d_ev.data_ptr(), stream=st)
    ani.set_ghost_fold(owner.data_ptr(), shift.data_ptr(), nt - nl)
    cap = 4096
    d_mol = torch.zeros(nl, dtype=torch.int32, device=dev)
    d_rows = torch.zeros((cap, len(sym) + 1), dtype=torch.int32, device=dev)
    d_sum = torch.zeros(6, dtype=torch.int64, device=dev)

    def step():
        ani.compute_device(nt, nl, 0, d_x.data_ptr(), inp.npairs, 0, 0, 0, 1, d_f.data_ptr(), d_ev.data_ptr(), stream=st)

    def find():
        ani.find_molecules_device(nt, nl, d_x.data_ptr(), None, d_mol.data_ptr(), d_rows.data_ptr(), cap, d_sum.data_ptr(), stream=st)

    def timed(fn, n):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    res = dict(ntotal=nt, nlocal=nl, npairs=int(inp.npairs), members=M, repulsion=rep, step_ms=[], find_molecules_ms=[])
    for r in range(2):
        res["step_ms"].append(timed(step, 50))
        res["find_molecules_ms"].append(timed(find, 500))
    torch.cuda.synchronize()
    s = d_sum.cpu().numpy()
    res["summary"] = dict(zip(ani_hip.SUMMARY_KEYS, s.tolist()))
    res["formulas"] = ani_hip.formula_dict(d_rows[: int(s[1])].cpu().numpy(), sym)
    res["find_over_step"] = min(res["find_molecules_ms"]) / min(res["step_ms"])
    print(name, json.dumps(res), flush=True)
    ani.close()
    out[name] = res
json.dump(out, open(sys.argv[1], "w"), indent=1)
