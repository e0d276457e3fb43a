"""GPU: the ensemble model deviation of include/ani_hip.h (ani_request_model_deviation) against fp64 references.

Definitions (pinned in the header): E_i^m the energy of centre i under member m (self energy included), F_j^m = -d(sum_i E_i^m)/dx_j
of the network part, dF^m = F^m - mean_m F^m, d_j = sqrt((1/M) sum_m |dF_j^m|^2) after the ghost rows are folded, sigma_E,i the
population standard deviation of E_i^m, member_energy[m] = sum_i E_i^m + the repulsion energy.  kcal/mol, kcal/mol/A.

References.  Every member m of a model file is written as a model file of its own (``AniModel`` with ``weights=[w_m]``, no
repulsion block: the repulsion is the same for every member and drops out of every deviation).
  fp64 handles   the oracle (``Oracle.compute``) on each single-member file: F^m, E_i^m, E^m; the repulsion energy is the full
                 model's energy minus the mean of the members' network energies.
  fp32 handles   two stages, each on the kernel's own input, so that a difference comes from the stage alone:
                 1. dE/dAEV: ``stage_reference.mlp_stage`` of each single-member model on the kernel's own AEV rows gives g_m and
                    its bar b_m (the per-member form: with one member the "members are summed" term kacc(M) u sum|g| is absent
                    from b_m); the ensemble's own mlp_stage gives the mean's bar b.  The kernel's dg_m = M p_m - mean, p_m the
                    member's rows scaled by 1/M, meets |dg_m - (g_m - mean g)| <= b_m + b + 3 u (|g_m| + |mean g|): the two
                    carried bars, plus the scale by 1/M and back (exact for M a power of two, one rounding otherwise) and the
                    final multiply-subtract.  Members' energies likewise from mlp_stage's eatom and eatom_bar.
                 2. the AEV backward: dF^m against ``Oracle.aev_vjp`` on the kernel's own dg_m rows (read through
                    ``ani_debug_deviation_parts``), with bar kappa u force_abs, force_abs the sum of the absolute values of
                    the terms of each force component.  kappa = kacc(n) + kx: kacc(n) = 8 sqrt(n) + 2 the probabilistic fp32
                    sum of n <= 3 (neighbours + 1)^2 (radial + angular shells) terms (stage_reference's accumulation model); kx the
                    fp32 positions, stored relative to the bounding box's midpoint: a difference d = x_j - x_i carries
                    |delta d| <= 2 u X (X the largest |x - midpoint|), and a term's relative change per unit of distance is
                    at most 2 eta Rc + 2 pi / Rc + 2 zeta / r_min (Gaussian, cosine cutoff, angular power; r_min the
                    shortest pair), so kx = 2 X (2 eta Rc + 2 pi / Rc + 2 zeta / r_min) per distance, times 2 for the two
                    distances of an angular term.
  d_j            |d - d_ref| <= max_m |e_m| with e_m the bar of |dF_j^m| (triangle inequality of the RMS norm over m).
  fp64           the 1e-8 kcal/mol/A of the fp64 forces (tests/test_atom_virial.py, F_TOL64) for each of F^m and the mean:
                 2e-8 per component; energies 1e-12 of sum |E_i| + 1e-8.
  armed/unarmed  the step's own outputs within the bars of tests/test_split_step.py (fp32 atomics in another order).
"""
import dataclasses
import math

import numpy as np
import pytest

from conftest import GOLDEN_CASES, golden_input, golden_model_path, load_golden
from lammps_ani_amd import harness as hx
from lammps_ani_amd import model_file as mf
import stage_reference as sr

pytestmark = pytest.mark.gpu

KCAL = 627.5094738898777
U = 2.0 ** -24
F_TOL64 = 1e-8
DEV_CASES = [c for c in GOLDEN_CASES]   # every golden fixture has M >= 2


@pytest.fixture(scope="module")
def hip():
    from lammps_ani_amd import ani_hip
    return ani_hip


@pytest.fixture(scope="module")
def member_files(tmp_path_factory):
    """model path -> [single-member model file without repulsion] (and the full model without repulsion)"""
    d = tmp_path_factory.mktemp("members")
    cache = {}

    def get(path):
        if path not in cache:
            m = mf.read_model(path)
            files = []
            for k in range(m.num_models):
                p = str(d / f"{len(cache)}_m{k}.anim")
                mf.write_model(p, dataclasses.replace(m, weights=[m.weights[k]], repulsion=None))
                files.append(p)
            cache[path] = (m, files)
        return cache[path]

    return get


def fold(a, inp):
    """ghost rows into their owners' rows (one periodic rank: every ghost is an image of an owned atom); axis 0"""
    out = a[: inp.nlocal].copy()
    np.add.at(out, np.asarray(inp.owner_lidx, dtype=np.int64), a[inp.nlocal:])
    return out


def oracle_members(path, inp, compat, member_files):
    """fp64: F[m] [ntotal, 3] (network part), eatom[m] [nlocal], E[m] total energies incl. repulsion"""
    from oracle import Oracle
    model, files = member_files(path)
    outs = [Oracle(p).compute(inp, radial_compat=compat) for p in files]
    F = np.stack([o["force"] for o in outs])
    ea = np.stack([o["eatom"] for o in outs])
    En = np.array([o["energy"] for o in outs])
    full = Oracle(path).compute(inp, radial_compat=compat)["energy"]
    return F, ea, En + (full - En.mean())


def kappa_backward(ani, inp, model):
    """kappa of stage 2 (module docstring), one per atom row"""
    x = np.asarray(inp.x, np.float64)
    X = float(np.abs(x - 0.5 * (x.max(0) + x.min(0))).max()) * math.sqrt(3.0)
    rcr, rca = ani.cutoffs()
    i = np.repeat(np.asarray(inp.ilist, np.int64), inp.numneigh)
    j = np.asarray(inp.jlist, np.int64)
    r = np.sqrt(((x[j] - x[i]) ** 2).sum(1))
    rmin = max(float(r[r > 0].min()), 0.5)
    eta = max(float(np.max(model.EtaR)), float(np.max(model.EtaA)))
    zeta = float(np.max(model.Zeta))
    rc = max(rcr, rca)
    kx = 2 * 2 * X * (2 * eta * rc + 2 * math.pi / rc + 2 * zeta / rmin)
    nn = np.bincount(j, minlength=inp.ntotal) + np.bincount(i, minlength=inp.ntotal) + 1
    nterms = 3 * nn ** 2 * (len(model.ShfR) + len(model.ShfA) * len(model.ShfZ))
    return np.array([sr.kacc(n) for n in nterms]) + kx


def kernel_parts(ani, inp, single):
    """the kernel's dg_m rows [M, nlocal, aev_len] (centre order, full width) and its AEV rows (full width)"""
    M = ani.use_num_models
    full, rows, v, cm = sr.full_width_rows(ani, inp.nlocal)
    p, stride = ani.debug_deviation_parts()
    dt = np.float32 if single else np.float64
    raw = ani.debug_read(p, (M * stride,), dt).reshape(M, stride)
    A = v.aev_active_length
    dg = np.zeros((M, inp.nlocal, ani.aev_length))
    for m in range(M):
        dg[m][:, cm] = raw[m][: v.nrows * v.aev_stride].reshape(v.nrows, v.aev_stride)[rows, :A]
    return dg, full


def stage_refs(model, files, aev_full, species, arith):
    """per-member mlp_stage on the kernel's AEV rows: g [M, n, A], bars, eatom [M, n], eatom bars; the ensemble's own bars"""
    M = model.num_models
    g, gb, ea, eab = [], [], [], []
    for k in range(M):
        o = sr.mlp_stage(dataclasses.replace(model, weights=[model.weights[k]], repulsion=None), aev_full, species, arith=arith)
        g.append(o["gaev"]); gb.append(o["gaev_bar"]); ea.append(o["eatom"]); eab.append(o["eatom_bar"])
    ens = sr.mlp_stage(dataclasses.replace(model, repulsion=None), aev_full, species, arith=arith)
    return np.stack(g), np.stack(gb), np.stack(ea), np.stack(eab), ens


def check_fp32(ani, inp, got, model, arith, compat, dev_fold=False, members=None):
    """stage 1 and stage 2 checks of an fp32 armed step (module docstring); returns the worst error / bar ratio"""
    from oracle import Oracle
    M = model.num_models
    species = np.asarray(inp.species)[np.asarray(inp.ilist)]
    dg, aev_full = kernel_parts(ani, inp, True)
    key = (ani_path_of(ani), arith, hash(aev_full.tobytes()))   # the forms and options share the forward: one reference per module
    if key not in _STAGE:
        _STAGE[key] = stage_refs(model, None, aev_full, species, arith)
    g, gb, ea, eab, ens = _STAGE[key]
    gm = g.mean(0)
    worst = 0.0
    # stage 1: dg_m
    # (on the columns the kernels run: those of species absent from the system are no AEV entries, their gradient is not formed)
    cm = ani.colmap()
    bar1 = gb + ens["gaev_bar"][None] + 3 * U * (np.abs(g) + np.abs(gm)[None]) + (0 if M in (1, 2, 4, 8, 16) else U * np.abs(g))
    bar1 = bar1[:, :, cm]
    err1 = np.abs(dg - (g - gm[None]))[:, :, cm]
    worst = max(worst, float((err1 / np.maximum(bar1, 1e-300)).max()))
    assert np.all(err1 <= bar1), (err1 / bar1).max()
    # energies: sigma_E and member_energy's spread (the repulsion and the self energies cancel in both)
    Em = ea                                  # [M, nlocal] kcal/mol incl. self energy
    ebar = eab + U * np.abs(Em)              # + the rescale by M of the 1/M-scaled rows
    sig_ref = np.sqrt(((Em - Em.mean(0)) ** 2).mean(0))
    sbar = ebar.max(0) + ebar.mean(0)
    err = np.abs(got["atom_energy_dev"] - sig_ref)
    assert np.all(err <= sbar), (err / sbar).max()
    me = got["member_energy"]
    Etot = Em.sum(1)
    mbar = ebar.sum(1) + ebar.mean(0).sum() + sr.kacc(inp.nlocal) * 1.2e-16 * np.abs(Em).sum(1)
    assert np.all(np.abs((me - me.mean()) - (Etot - Etot.mean())) <= mbar)
    # stage 2: dF^m on the kernel's own dg_m
    o = Oracle(network_only(ani_path_of(ani)))   # aev_vjp takes no repulsion block; dg has none
    kap = kappa_backward(ani, inp, model)[:, None]
    # pairs within the position error 2 u X of a cutoff are in for one side and out for the other: such a term is at most
    # sum_c |dg_c| * fc'(Rc - 2 u X) ~ sum_c |dg_c| (pi / Rc)^2 u X, four of them per row
    x = np.asarray(inp.x, np.float64)
    X = float(np.abs(x - 0.5 * (x.max(0) + x.min(0))).max()) * math.sqrt(3.0)
    floor = 4 * KCAL * (math.pi / min(ani.cutoffs())) ** 2 * U * X
    dF = got["member_dforce"]                # [ntotal, M, 3]
    refs, bars = [], []
    for m in (members if members is not None else range(M)):
        r = o.aev_vjp(inp, dg[m], radial_compat=compat)
        bar = kap * U * r["force_abs"] + floor * np.abs(dg[m]).sum(1).max()
        refs.append(r["force"]); bars.append(bar)
        if dev_fold:
            ref, b = fold(r["force"], inp), fold(bar, inp)
            e2 = np.abs(dF[: inp.nlocal, m] - ref)
        else:
            ref, b = r["force"], bar
            e2 = np.abs(dF[:, m] - ref)
        worst = max(worst, float((e2 / b).max()))
        assert np.all(e2 <= b), (m, (e2 / b).max())
    return worst, refs, bars


_PATHS = {}
_STAGE = {}
_NET = {}


def network_only(path):
    """the model file without its repulsion block (the same file when it has none)"""
    if path not in _NET:
        m = mf.read_model(path)
        if m.repulsion is None:
            _NET[path] = path
        else:
            q = path + ".net.anim"
            mf.write_model(q, dataclasses.replace(m, repulsion=None))
            _NET[path] = q
    return _NET[path]


def ani_path_of(ani):
    return _PATHS[id(ani)]


def make_ani(hip, path, **kw):
    ani = hip.ANI(path, 0, -1, **kw)
    _PATHS[id(ani)] = path
    return ani


def d_from(dF_rows, nlocal, inp, folded):
    """d_j of [rows, M, 3] rows (folded into owners when not yet)"""
    f = dF_rows if folded else fold(dF_rows, inp)
    return np.sqrt((f[:nlocal] ** 2).sum(2).mean(1))


# ---- 1. against fp64 references, every golden fixture -----------------------------------------------------------------
@pytest.mark.parametrize("case", DEV_CASES)
@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("single", [True, False], ids=["fp32", "fp64"])
def test_deviation_matches_reference(case, half, single, model_cache, member_files, hip):
    g = load_golden(case)
    inp = golden_input(g, half=half)
    path = golden_model_path(g, model_cache)
    model = mf.read_model(path)
    M = model.num_models
    nt, nl = inp.ntotal, inp.nlocal
    ani = make_ani(hip, path, use_fullnbr=not half, use_single=single)
    got = ani.compute(inp, ago=0, deviation=True)
    dv = got["deviation"]
    assert dv["member_energy"].shape == (M,) and dv["member_dforce"].shape == (nt, M, 3)
    assert abs(dv["member_energy"].mean() - got["energy"]) < (1e-3 if single else 1e-7) * max(1.0, nl / 10)
    # the members' deviations sum to zero over m
    assert np.abs(dv["member_dforce"].sum(1)).max() < (1e-3 if single else 1e-8)
    if single:
        worst, refs, bars = check_fp32(ani, inp, dv, model, 1, False)
        if nt == nl:
            dref = np.sqrt((np.stack(refs, 1) ** 2).sum(2).mean(1))
            err = np.abs(dv["atom_force_dev"] - dref)
            assert np.all(err <= np.stack(bars, 1).max(1).max(1))
        else:
            # host entry with ghosts: fold member_dforce here and check the d that results
            d = d_from(dv["member_dforce"], nl, inp, False)
            dref = np.sqrt((np.stack([fold(r, inp) for r in refs], 1) ** 2).sum(2).mean(1))
            bmax = np.stack([fold(b, inp) for b in bars], 1).max(1).max(1)
            assert np.all(np.abs(d - dref) <= bmax)
        print(f"{case}/{'half' if half else 'full'}/fp32: worst error/bar {worst:.3g}")
    else:
        F, ea, E = oracle_members(path, inp, False, member_files)
        dref = F - F.mean(0)[None]                                 # [M, nt, 3]
        assert np.abs(dv["member_dforce"].transpose(1, 0, 2) - dref).max() <= 2 * F_TOL64
        sig = np.sqrt(((ea - ea.mean(0)) ** 2).mean(0))
        ebar = 1e-12 * np.abs(ea).max() + 1e-8
        assert np.abs(dv["atom_energy_dev"] - sig).max() <= ebar
        assert np.abs(dv["member_energy"] - E).max() <= 1e-12 * np.abs(ea).sum() + 1e-8
        dj = d_from(dref.transpose(1, 0, 2), nl, inp, nt == nl)
        if nt == nl:
            assert np.abs(dv["atom_force_dev"] - dj).max() <= 2 * F_TOL64
            s = dv["summary"]
            assert abs(s[0] - dj.max()) <= 2 * F_TOL64 and abs(s[1] - dj.min()) <= 2 * F_TOL64
            assert abs(s[2] - dj.sum()) <= 2 * F_TOL64 * nl and abs(s[3] - sig.max()) <= ebar
        else:
            assert np.abs(d_from(dv["member_dforce"], nl, inp, False) - dj).max() <= 4 * F_TOL64
    ani.close()


def test_open_fixture_summary_and_modes(model_cache, member_files, hip):
    """The open fixture (no ghosts) through the host entry: atom_force_dev and summary; cuaev and pyaev (compat) modes."""
    case = "water30_open_ani2x_m8"
    g = load_golden(case)
    inp = golden_input(g)
    path = golden_model_path(g, model_cache)
    model = mf.read_model(path)
    for mode in ("strict", "compat"):
        ani = make_ani(hip, path, use_cuaev=(mode == "strict"))
        dv = ani.compute(inp, ago=0, deviation=True)["deviation"]
        _, refs, bars = check_fp32(ani, inp, dv, model, 1, mode == "compat")
        dref = np.sqrt((np.stack(refs, 1) ** 2).sum(2).mean(1))
        bmax = np.stack(bars, 1).max(1).max(1)
        assert np.all(np.abs(dv["atom_force_dev"] - dref) <= bmax)
        s = dv["summary"]
        d = dv["atom_force_dev"]
        assert s[0] == d.max() and s[1] == d.min() and abs(s[2] - d.sum()) <= 1e-12 * d.sum()
        assert s[3] == dv["atom_energy_dev"].max()
        ani.close()


def _dev(inp, torch, dev):
    return dict(x=torch.from_numpy(inp.x.reshape(-1).copy()).to(dev), species=torch.from_numpy(inp.species.astype(np.int32)).to(dev),
                ilist=torch.from_numpy(inp.ilist).to(dev), numneigh=torch.from_numpy(inp.numneigh).to(dev),
                jlist=torch.from_numpy(inp.jlist).to(dev))


def device_step(ani, inp, torch, dev, fold_on, keys=("member_energy", "atom_energy_dev", "member_dforce", "atom_force_dev", "summary")):
    nt, nl = inp.ntotal, inp.nlocal
    M = ani.use_num_models
    d = _dev(inp, torch, dev)
    f = torch.zeros(nt * 3, dtype=torch.float64, device=dev)
    ev = torch.zeros(10, dtype=torch.float64, device=dev)
    ani.compute_device(nt, nl, d["species"].data_ptr(), d["x"].data_ptr(), inp.npairs, d["ilist"].data_ptr(), d["jlist"].data_ptr(),
                       d["numneigh"].data_ptr(), 0, f.data_ptr(), ev.data_ptr())
    keep = []
    if fold_on:
        owner = torch.from_numpy(np.asarray(inp.owner_lidx, dtype=np.int64)).to(dev)
        shift = torch.from_numpy((inp.x[nl:] - inp.x[np.asarray(inp.owner_lidx)]).reshape(-1).copy()).to(dev)
        ani.set_ghost_fold(owner.data_ptr(), shift.data_ptr(), nt - nl)
        keep = [owner, shift]
    shapes = dict(member_energy=(M,), atom_energy_dev=(nl,), member_dforce=(nt, M, 3), atom_force_dev=(nl,), summary=(4,))
    out = {k: torch.full(shapes[k], float("nan"), dtype=torch.float64, device=dev) for k in keys}
    f.zero_(); ev.zero_()
    ani.compute_device(nt, nl, 0, d["x"].data_ptr(), inp.npairs, 0, 0, 0, 1, f.data_ptr(), ev.data_ptr(),
                       d_deviation={k: v.data_ptr() for k, v in out.items()})
    torch.cuda.synchronize()
    del keep
    return {k: v.cpu().numpy() for k, v in out.items()}, float(ev[0].item())


@pytest.mark.parametrize("case", [c for c in DEV_CASES if "pbc" in c])
def test_device_entry_with_ghost_fold(case, model_cache, hip):
    """pbc fixtures through ani_compute_full_device with the ghost fold (fp32): folded member_dforce rows, their ghost rows keep
    the NaN sentinels, atom_force_dev and summary."""
    import torch
    dev = torch.device("cuda:0")
    g = load_golden(case)
    inp = golden_input(g)
    path = golden_model_path(g, model_cache)
    model = mf.read_model(path)
    nl = inp.nlocal
    ani = make_ani(hip, path)
    dv, e = device_step(ani, inp, torch, dev, True)
    assert np.all(np.isnan(dv["member_dforce"][nl:]))
    _, refs, bars = check_fp32(ani, inp, dv, model, 1, False, dev_fold=True)
    dref = np.sqrt((np.stack([fold(r, inp) for r in refs], 1) ** 2).sum(2).mean(1))
    bmax = np.stack([fold(b, inp) for b in bars], 1).max(1).max(1)
    assert np.all(np.abs(dv["atom_force_dev"] - dref) <= bmax)
    s, d = dv["summary"], dv["atom_force_dev"]
    assert s[0] == d.max() and s[1] == d.min() and abs(s[2] - d.sum()) <= 1e-12 * d.sum() and s[3] == dv["atom_energy_dev"].max()
    assert abs(dv["member_energy"].mean() - e) < 1e-3 * max(1.0, nl / 10)
    ani.close()


# ---- 2. the 10 002-water x 8 box under every form and option of the armed path ------------------------------------------
OPTIONS = [("default", None, None), ("gen0", "mlp_fused_gen", 0), ("fused3", "mlp_fused", 3), ("fused0", "mlp_fused", 0),
           ("arith2", "mlp_arith", 2), ("arith0", "mlp_arith", 0), ("tickets", "aev_tickets_min", 0), ("sym0", "aev_symmetric_radial", 0)]
_BOX = {}


def water_box_ref(model_cache):
    if not _BOX:
        p = model_cache("ani2x", 8, 2024)
        inp = hx.decompose(hx.spatial_sort(hx.water_box(10002, seed=12345)))
        _BOX.update(path=p, inp=inp, model=mf.read_model(p), stage={})
    return _BOX


@pytest.mark.parametrize("opt", OPTIONS, ids=[o[0] for o in OPTIONS])
def test_water_box_options(opt, model_cache, hip):
    box = water_box_ref(model_cache)
    inp, model = box["inp"], box["model"]
    ani = make_ani(hip, box["path"])
    if opt[1]:
        ani.set_option(opt[1], opt[2])
    got = ani.compute(inp, ago=0, deviation=True)
    dv = got["deviation"]
    arith = 2 if opt[0] == "arith2" else 1
    # members 0 and 7 through the oracle's backward (each aev_vjp is a pass over the box); stage 1 covers all eight
    worst, refs, bars = check_fp32(ani, inp, dv, model, arith, False, members=[0, 7])
    d = d_from(dv["member_dforce"], inp.nlocal, inp, False)
    assert np.all(np.isfinite(d)) and d.max() > 0
    assert abs(dv["member_energy"].mean() - got["energy"]) < 1e-6 * abs(got["energy"]) + 1.0
    print(f"water 10002 x 8 / {opt[0]}: kernel {ani.last_mlp_kernel()}, worst error/bar {worst:.3g}")
    ani.close()


# ---- 3. arming changes nothing else --------------------------------------------------------------------------------------
def test_armed_step_changes_nothing_else(model_cache, hip):
    g = load_golden("mixed64_pbc_ani1x_m2_rep")
    inp = golden_input(g)
    ani = make_ani(hip, golden_model_path(g, model_cache))
    plain = ani.compute(inp, ago=0, atom_virial=9)
    armed = ani.compute(inp, ago=1, atom_virial=9, deviation=True)
    fmax = float(np.abs(plain["force"]).max())
    assert np.abs(armed["force"] - plain["force"]).max() < 2e-4 + 2e-6 * fmax
    assert abs(armed["energy"] - plain["energy"]) < 1e-3
    assert np.abs(armed["virial"] - plain["virial"]).max() < 1e-5 * np.abs(plain["virial"]).max() + 1e-2
    assert np.abs(armed["eatom"] - plain["eatom"]).max() < 1e-3
    assert np.abs(armed["atom_virial"] - plain["atom_virial"]).max() < 1e-5 * np.abs(plain["atom_virial"]).max() + 1e-2
    # one repeat of the same armed step agrees within the atomics-order bar (scratch cleared between members and steps)
    again = ani.compute(inp, ago=1, deviation=True)["deviation"]
    a = armed["deviation"]
    assert np.abs(again["member_dforce"] - a["member_dforce"]).max() < 2e-4 + 2e-6 * float(np.abs(a["member_dforce"]).max())
    assert np.array_equal(again["atom_energy_dev"], a["atom_energy_dev"])
    assert np.array_equal(again["member_energy"], a["member_energy"])
    # the next, unarmed step writes nothing to the arrays of the armed one
    outs = dict(member_energy=np.full(2, 7.0), atom_energy_dev=np.full(inp.nlocal, 7.0), member_dforce=np.full((inp.ntotal, 2, 3), 7.0))
    ani.request_model_deviation(**outs)
    ani.compute(inp, ago=1)
    snap = {k: v.copy() for k, v in outs.items()}
    ani.compute(inp, ago=1)
    for k in outs:
        assert np.array_equal(outs[k], snap[k])
    ani.close()


def test_energy_only_arming(model_cache, hip):
    """member_energy / atom_energy_dev alone: no force output, the same values as a force-armed step."""
    g = load_golden("water30_pbc_ani2x_m8")
    inp = golden_input(g)
    ani = make_ani(hip, golden_model_path(g, model_cache))
    full = ani.compute(inp, ago=0, deviation=True)["deviation"]
    me, ae = np.full(8, np.nan), np.full(inp.nlocal, np.nan)
    ani.request_model_deviation(member_energy=me, atom_energy_dev=ae)
    ani.compute(inp, ago=1)
    assert np.array_equal(me, full["member_energy"]) and np.array_equal(ae, full["atom_energy_dev"])
    ani.close()


# ---- 4. member structure ---------------------------------------------------------------------------------------------------
def test_permuted_and_identical_members(model_cache, tmp_path, hip):
    g = load_golden("water30_open_ani2x_m8")
    inp = golden_input(g)
    path = golden_model_path(g, model_cache)
    model = mf.read_model(path)
    perm = [3, 0, 7, 5, 1, 6, 2, 4]
    pp = str(tmp_path / "perm.anim")
    mf.write_model(pp, dataclasses.replace(model, weights=[model.weights[k] for k in perm]))
    base = make_ani(hip, path).compute(inp, ago=0, deviation=True)["deviation"]
    per = make_ani(hip, pp).compute(inp, ago=0, deviation=True)["deviation"]
    # member energies permute (fp32 sums in another member order: 8 members' rounding)
    ebar = 8 * sr.kacc(inp.nlocal) * U * np.abs(base["member_energy"]).max()
    assert np.abs(per["member_energy"] - base["member_energy"][perm]).max() <= ebar
    assert np.abs(per["atom_energy_dev"] - base["atom_energy_dev"]).max() <= 1e-5 * max(1.0, base["atom_energy_dev"].max())
    assert np.abs(per["atom_force_dev"] - base["atom_force_dev"]).max() <= 1e-3 * max(1.0, base["atom_force_dev"].max())
    assert np.abs(per["member_dforce"] - base["member_dforce"][:, perm]).max() <= 1e-3 * max(1.0, np.abs(base["member_dforce"]).max())
    # M identical members: every deviation is rounding.  The members' rows are the same bits, so the energies agree exactly up
    # to the fp64 mean (sigma_E <= 4 2^-52 |E_i| < 1e-10 for |E_i| < 1e5 kcal/mol); the fp32 mean of the dE/dAEV rows is off by
    # at most two roundings and the multiply-subtract by one: |dg| <= 3 u |g|, whose backward pass is bounded by 3 u force_abs
    # of g (plus its own rounding, a factor 1 + kappa u).
    from oracle import Oracle
    pi = str(tmp_path / "same.anim")
    mf.write_model(pi, dataclasses.replace(model, weights=[model.weights[0]] * 4))
    same = make_ani(hip, pi).compute(inp, ago=0, deviation=True)["deviation"]
    assert np.ptp(same["member_energy"]) == 0.0
    assert same["atom_energy_dev"].max() <= 1e-10
    o = Oracle(pi)
    fabs = o.aev_vjp(inp, np.abs(o.compute(inp, want_aev=True)["gaev"]))["force_abs"]
    bar = 4 * U * fabs
    assert np.all(np.abs(same["member_dforce"]) <= bar[:, None, :])
    assert same["summary"][0] <= np.sqrt((bar ** 2).sum(1)).max()


# ---- 5. contract errors ----------------------------------------------------------------------------------------------------
def test_contract_errors(model_cache, hip):
    import torch
    g = load_golden("water30_pbc_ani2x_m8")
    inp = golden_input(g)
    path = golden_model_path(g, model_cache)
    # one member: refused, unarmed, the next step runs
    one = hip.ANI(path, 0, 1)
    with pytest.raises(hip.AniError, match="at least 2"):
        one.request_model_deviation(member_energy=np.zeros(1))
    assert np.isfinite(one.compute(inp, ago=0)["energy"])
    one.close()
    ani = make_ani(hip, path)
    # atom_force_dev on a host step with ghosts: refused, names the fold; the arming is consumed
    ani.request_model_deviation(atom_force_dev=np.zeros(inp.nlocal))
    with pytest.raises(hip.AniError, match="fold"):
        ani.compute(inp, ago=0)
    got = ani.compute(inp, ago=0)
    assert np.isfinite(got["energy"]) and "deviation" not in got
    # an armed split step
    dev = torch.device("cuda:0")
    d = _dev(inp, torch, dev)
    f = torch.zeros(inp.ntotal * 3, dtype=torch.float64, device=dev)
    ev = torch.zeros(10, dtype=torch.float64, device=dev)
    ani.compute_device(inp.ntotal, inp.nlocal, d["species"].data_ptr(), d["x"].data_ptr(), inp.npairs, d["ilist"].data_ptr(),
                       d["jlist"].data_ptr(), d["numneigh"].data_ptr(), 0, f.data_ptr(), ev.data_ptr())
    me = torch.zeros(8, dtype=torch.float64, device=dev)
    ani.request_model_deviation(member_energy=me.data_ptr())
    with pytest.raises(hip.AniError, match="split step"):
        ani.step_begin(inp.ntotal, inp.nlocal, d["x"].data_ptr(), f.data_ptr(), ev.data_ptr())
    # all NULL disarms
    out = np.full(8, 7.0)
    ani.request_model_deviation(member_energy=out)
    ani.request_model_deviation()
    ani.compute(inp, ago=0)
    assert np.all(out == 7.0)
    # a communicator attached: no force output on the host entries
    nat = hip.NativeComm(1, 0, hip.NativeComm.unique_id(), 0)
    ani.attach_comm(nat)
    ani.request_model_deviation(member_dforce=np.zeros((inp.ntotal, 8, 3)))
    with pytest.raises(hip.AniError, match="communicator"):
        ani.compute(inp, ago=0)
    ani.attach_comm(None)
    ani.close()
    nat.close()
