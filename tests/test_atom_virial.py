"""GPU: the per-atom virial of include/ani_hip.h (ani_request_atom_virial) against an fp64 reference built from the oracle.

Definition (site-energy form, pinned in the header): W_j = sum over centres i with j in their list of (x_j - x_i) (x) F_j^(i),
F_j^(i) = -dE_i/dx_j, "xy" = sum (x_j - x_i)_x F_y, kcal/mol.  ncomp 9 is LAMMPS' cvatom order (xx yy zz xy xz yz yx zx zy), 6 the
vatom order of the symmetric part.

Reference: F^(i) of every centre from Oracle.aev_vjp with every dE/dAEV row zeroed except centre i's (the true rows from
compute(want_aev=True)); for repulsion models (aev_vjp refuses them) the same network without the repulsion block (the synthetic
generator appends it after the networks of the same seed) plus the half-pair term of every list entry, restated in
tests/repulsion_reference.py from oracle/ani_oracle.c:rep_pair.  One small open fixture is cross-checked against central differences of the oracle's eatom.

Bars, derived from the bars the forces already meet (tests/test_hip_parity.py):
  fp32 handle   a row's component is a sum of at most n_j terms (x_j - x_i)_a F_b, |x_j - x_i| <= Rcr, each F off by at most
                F_TOL = 2.3e-3 kcal/mol/A  ->  |dW_j| <= Rcr * F_TOL * n_j.
  fp64 handle   the same with the 1e-8 kcal/mol/A the fp64 forces reach  ->  |dW_j| <= Rcr * 1e-8 * n_j.
  sums          sum_j W_j and out_virial are two fp32 sums of the same terms, each within the parity test's virial bar of the fp64
                value: their symmetric parts differ by at most 2 * V_TOL * max(1, natoms / 100), V_TOL = 2e-2 kcal/mol.
  armed/unarmed the same arithmetic with fp32 atomics in another order: the bars of tests/test_split_step.py.
"""
import numpy as np
import pytest

from conftest import GOLDEN_CASES, golden_input, golden_model_path, load_golden
from lammps_ani_amd import harness as hx
from lammps_ani_amd import model_file as mf
from repulsion_reference import rep_terms

pytestmark = pytest.mark.gpu

KCAL = 627.5094738898777
F_TOL = 2.3e-3
F_TOL64 = 1e-8
V_TOL = 2e-2
CVATOM = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2), (1, 0), (2, 0), (2, 1)]


@pytest.fixture(scope="module")
def hip():
    from lammps_ani_amd import ani_hip
    return ani_hip


def to_ncomp(W, ncomp):
    """[n, 3, 3] -> [n, ncomp] in LAMMPS order"""
    if ncomp == 9:
        return np.stack([W[:, a, b] for a, b in CVATOM], axis=1)
    S = 0.5 * (W + W.transpose(0, 2, 1))
    return np.stack([S[:, a, b] for a, b in CVATOM[:6]], axis=1)


def fold(W, inp):
    """ghost rows into their owners' rows (one periodic rank: every ghost is an image of an owned atom)"""
    out = W[: inp.nlocal].copy()
    np.add.at(out, np.asarray(inp.owner_lidx, dtype=np.int64), W[inp.nlocal:])
    return out


def reference(g, inp_full, model_cache, compat):
    """fp64 site-energy per-atom virial W[ntotal, 3, 3], the number of terms per row, and the reference forces' total"""
    from oracle import Oracle
    rep_model = bool(int(g["repulsion"])) if "repulsion" in g else False
    p = model_cache(str(g["kind"]), int(g["num_models"]), int(g["seed"]), False)
    o = Oracle(p)
    base = o.compute(inp_full, radial_compat=compat, want_aev=True)
    nt, nl = inp_full.ntotal, inp_full.nlocal
    W = np.zeros((nt, 3, 3))
    nterm = np.zeros(nt, dtype=np.int64)
    ftot = np.zeros((nt, 3))
    for c in range(nl):
        gz = np.zeros_like(base["gaev"])
        gz[c] = base["gaev"][c]
        F = o.aev_vjp(inp_full, gz, radial_compat=compat)["force"]
        ftot += F
        ci = int(inp_full.ilist[c])
        d = inp_full.x - inp_full.x[ci]
        W += d[:, :, None] * F[:, None, :]
        nterm += np.any(F != 0.0, axis=1) & (np.arange(nt) != ci)
    if rep_model:
        rep = mf.read_model(golden_model_path(g, model_cache)).repulsion
        i, j, d, gv = rep_terms(inp_full, rep)
        F = -KCAL * gv
        np.add.at(W, j, d[:, :, None] * F[:, None, :])
        np.add.at(ftot, j, F)
        np.add.at(ftot, i, -F)
        np.add.at(nterm, j, (gv != 0).any(1).astype(np.int64))
    # self-check: the per-centre forces (and the repulsion entries) add up to the fixture's forces
    assert np.abs(ftot - g[f"{'compat' if compat else 'strict'}_force"]).max() < 1e-7
    return W, np.maximum(nterm, 1), ftot


_REF = {}


def cached_reference(case, mode, model_cache):
    key = (case, mode)
    if key not in _REF:
        g = load_golden(case)
        _REF[key] = reference(g, golden_input(g), model_cache, mode == "compat")
    return _REF[key]


def test_central_differences(model_cache, hip):
    """Fully independent reference on the open 30-atom water (no ghosts): central differences of the oracle's eatom over every
    coordinate.  h = 1e-4 A: truncation h^2 |third derivative| / 6 ~ 1e-6 kcal/mol/A per force, rounding 1e-16 |E_i| / h ~ 5e-7,
    so each difference force is good to 1e-5 and a row to Rcr * 1e-5 * n_j.  The aev_vjp reference, and the fp64 handle, meet
    that bar against it; the reference's sum over rows is the fixture's global virial."""
    from oracle import Oracle
    case = "water30_open_ani2x_m8"
    g = load_golden(case)
    inp = golden_input(g)
    W_ref, n, _ = cached_reference(case, "strict", model_cache)
    o = Oracle(golden_model_path(g, model_cache))
    nt, nl, h = inp.ntotal, inp.nlocal, 1e-4
    x0 = inp.x.copy()
    dE = np.zeros((nl, nt, 3))   # dE_i / dx_j
    for j in range(nt):
        for k in range(3):
            for sgn in (1.0, -1.0):
                inp.x[:] = x0
                inp.x[j, k] += sgn * h
                dE[:, j, k] += sgn * o.compute(inp)["eatom"] / (2 * h)
    inp.x[:] = x0
    W = np.zeros((nt, 3, 3))
    for c in range(nl):
        ci = int(inp.ilist[c])
        W += (x0 - x0[ci])[:, :, None] * (-dE[c])[:, None, :]
    bar = (5.2 * 1e-5 * n)[:, None, None]
    assert np.all(np.abs(W - W_ref) <= bar)
    S = W_ref.sum(0)
    assert np.abs(0.5 * (S + S.T) - g["strict_virial"]).max() < 1e-6 * max(1.0, np.abs(g["strict_virial"]).max())
    ani = hip.ANI(golden_model_path(g, model_cache), 0, use_single=False)
    got = ani.compute(inp, ago=0, atom_virial=9)["atom_virial"]
    assert np.all(np.abs(got - to_ncomp(W, 9)) <= bar[:, :, 0] + (5.2 * F_TOL64 * n)[:, None])
    ani.close()


@pytest.mark.parametrize("case", GOLDEN_CASES)
@pytest.mark.parametrize("mode", ["strict", "compat"])
@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("single", [True, False], ids=["fp32", "fp64"])
def test_atom_virial_matches_reference(case, mode, half, single, model_cache, hip):
    g = load_golden(case)
    inp = golden_input(g, half=half)
    W_ref, n, _ = cached_reference(case, mode, model_cache)
    ani = hip.ANI(golden_model_path(g, model_cache), 0, -1, use_cuaev=(mode == "strict"), use_fullnbr=not half, use_single=single)
    rcr = ani.cutoffs()[0]
    bar = (rcr * (F_TOL if single else F_TOL64) * n)[:, None]
    for ncomp in (9, 6):
        got = ani.compute(inp, ago=0, atom_virial=ncomp)
        assert got["atom_virial"].shape == (inp.ntotal, ncomp)
        err = np.abs(got["atom_virial"] - to_ncomp(W_ref, ncomp))
        print(f"{case}/{mode}/{'half' if half else 'full'}/{'fp32' if single else 'fp64'}/{ncomp}: max err {err.max():.2e}, "
              f"max |W| {np.abs(W_ref).max():.2e}")
        assert np.all(err <= bar), (err / bar).max()
        # its own sum against its own global virial
        S = np.zeros((3, 3))
        av = got["atom_virial"].sum(0)
        if ncomp == 9:
            for c, (a, b) in enumerate(CVATOM):
                S[a, b] = av[c]
            S = 0.5 * (S + S.T)
        else:
            for c, (a, b) in enumerate(CVATOM[:6]):
                S[a, b] = S[b, a] = av[c]
        assert np.abs(S - got["virial"]).max() < 2 * V_TOL * max(1.0, inp.nlocal / 100.0)
    ani.close()


@pytest.mark.parametrize("opt", ["default", "sym0", "fused0", "tickets"])
def test_atom_virial_options(opt, model_cache, hip):
    """The symmetric radial collection off, the two-kernel forward, rows by ticket: the same per-atom virial.  The fixture has
    rows with W_xy != W_yx by far more than the bar, so the orientation of the 9-component form is pinned."""
    case = "mixed96_pbc_ani2x_m2"
    g = load_golden(case)
    inp = golden_input(g)
    W_ref, n, _ = cached_reference(case, "strict", model_cache)
    ani = hip.ANI(golden_model_path(g, model_cache), 0)
    if opt != "default":
        ani.set_option({"sym0": "aev_symmetric_radial", "fused0": "aev_fused", "tickets": "aev_tickets_min"}[opt],
                       1 if opt == "tickets" else 0)
    got = ani.compute(inp, ago=0, atom_virial=9)["atom_virial"]
    bar = ani.cutoffs()[0] * F_TOL * n
    assert np.all(np.abs(got - to_ncomp(W_ref, 9)) <= bar[:, None])
    assert np.any(np.abs(W_ref[:, 0, 1] - W_ref[:, 1, 0]) > 4 * bar)
    assert np.any(np.abs(got[:, 3] - got[:, 6]) > 2 * bar)
    ani.close()


def _dev(inp, torch, dev):
    return dict(x=torch.from_numpy(inp.x.reshape(-1).copy()).to(dev), species=torch.from_numpy(inp.species.astype(np.int32)).to(dev),
                ilist=torch.from_numpy(inp.ilist).to(dev), numneigh=torch.from_numpy(inp.numneigh).to(dev),
                jlist=torch.from_numpy(inp.jlist).to(dev))


@pytest.mark.parametrize("entry,single", [("device", True), ("device", False), ("device_overwrite", True), ("device_fold", True),
                                          ("split", True), ("split", False)])
def test_device_entries(entry, single, model_cache, hip):
    """Device entries: added in place like d_f (written under device_overwrite_forces); with a ghost fold the ghost rows fold
    into their owners and are not written; the split step adds both halves and ani_step_finish writes."""
    import torch
    dev = torch.device("cuda:0")
    case = "mixed96_pbc_ani2x_m2"
    g = load_golden(case)
    inp = golden_input(g)
    W_ref, n, _ = cached_reference(case, "strict", model_cache)
    ref9 = to_ncomp(W_ref, 9)
    bar = (5.2 * (F_TOL if single else F_TOL64) * n)[:, None]
    nt, nl = inp.ntotal, inp.nlocal
    d = _dev(inp, torch, dev)
    ani = hip.ANI(golden_model_path(g, model_cache), 0, use_single=single)
    f = torch.zeros(nt * 3, dtype=torch.float64, device=dev)
    ev = torch.zeros(10, dtype=torch.float64, device=dev)
    ani.compute_device(nt, nl, d["species"].data_ptr(), d["x"].data_ptr(), inp.npairs, d["ilist"].data_ptr(), d["jlist"].data_ptr(),
                       d["numneigh"].data_ptr(), 0, f.data_ptr(), ev.data_ptr(), vflag=True)
    start = torch.full((nt, 9), 1.5, dtype=torch.float64, device=dev)   # added to, unless overwritten
    av = start.clone()
    if entry == "device_overwrite":
        ani.set_option("device_overwrite_forces", 1)
    if entry == "device_fold":
        owner = torch.from_numpy(np.asarray(inp.owner_lidx, dtype=np.int64)).to(dev)
        shift = torch.from_numpy((inp.x[nl:] - inp.x[np.asarray(inp.owner_lidx)]).reshape(-1).copy()).to(dev)
        ani.set_ghost_fold(owner.data_ptr(), shift.data_ptr(), nt - nl)
    if entry == "split":
        ani.step_begin(nt, nl, d["x"].data_ptr(), f.data_ptr(), ev.data_ptr(), vflag=True, d_atom_virial=av.data_ptr(), ncomp=9)
        ani.step_ghosts_ready()
        ani.step_finish()
    else:
        ani.compute_device(nt, nl, 0, d["x"].data_ptr(), inp.npairs, 0, 0, 0, 1, f.data_ptr(), ev.data_ptr(), vflag=True,
                           d_atom_virial=av.data_ptr(), ncomp=9)
    torch.cuda.synchronize()
    got = av.cpu().numpy()
    if entry == "device_fold":
        assert np.all(got[nl:] == 1.5)                         # ghost rows not written
        ref, b = fold(ref9, inp), fold(bar, inp)
        assert np.all(np.abs(got[:nl] - 1.5 - ref) <= b)
    elif entry == "device_overwrite":
        assert np.all(np.abs(got - ref9) <= bar)
    else:
        assert np.all(np.abs(got - 1.5 - ref9) <= bar)
    ani.close()


def test_armed_step_changes_nothing_else_and_disarms(model_cache, hip):
    """An armed call returns the energy, forces and global virial of an unarmed one (fp32 atomics in another order); the next
    unarmed call leaves the array alone."""
    g = load_golden("mixed64_pbc_ani1x_m2_rep")
    inp = golden_input(g)
    ani = hip.ANI(golden_model_path(g, model_cache), 0)
    plain = ani.compute(inp, ago=0)
    armed = ani.compute(inp, ago=1, atom_virial=9)
    fmax = float(np.abs(plain["force"]).max())
    assert np.abs(armed["force"] - plain["force"]).max() < 2e-4 + 2e-6 * fmax
    assert abs(armed["energy"] - plain["energy"]) < 1e-3
    assert np.abs(armed["virial"] - plain["virial"]).max() < 1e-5 * np.abs(plain["virial"]).max() + 1e-2
    out = np.full((inp.ntotal, 9), 7.0)
    ani.request_atom_virial(out, 9)
    ani.compute(inp, ago=1)
    snap = out.copy()
    ani.compute(inp, ago=1)
    assert np.array_equal(out, snap)
    ani.close()


def test_bad_requests_are_refused(model_cache, hip):
    g = load_golden("water30_pbc_ani2x_m8")
    inp = golden_input(g)
    ani = hip.ANI(golden_model_path(g, model_cache), 0)
    out = np.zeros((inp.ntotal, 5))
    with pytest.raises(hip.AniError, match="ncomp"):
        ani.request_atom_virial(out, 5)
    nat = hip.NativeComm(1, 0, hip.NativeComm.unique_id(), 0)
    ani.attach_comm(nat)
    with pytest.raises(hip.AniError, match="communicator"):
        ani.compute(inp, ago=0, atom_virial=9)
    ani.attach_comm(None)
    got = ani.compute(inp, ago=0, atom_virial=6)   # detached: fine again
    assert np.all(np.isfinite(got["atom_virial"]))
    ani.close()
    nat.close()


def test_water_box_sum_translation_finite(model_cache, hip):
    """12 501 water atoms (periodic, one rank): every value finite, sum_j vatom_j = out_virial of the same call, and a rigid
    translation of every coordinate leaves W unchanged (bar: twice the fp32 per-row bar, both sides are fp32 results)."""
    p = model_cache("ani2x", 1, 2024)
    sysm = hx.spatial_sort(hx.water_box(12501, seed=12345))
    inp = hx.decompose(sysm)
    ani = hip.ANI(p, 0)
    got = ani.compute(inp, ago=0, atom_virial=6)
    av = got["atom_virial"]
    assert np.all(np.isfinite(av))
    s = av.sum(0)
    V = got["virial"]
    sym = np.array([V[0, 0], V[1, 1], V[2, 2], V[0, 1], V[0, 2], V[1, 2]])
    assert np.abs(s - sym).max() < 2 * V_TOL * max(1.0, inp.nlocal / 100.0)
    nmax = int(np.max(inp.numneigh))
    ani2 = hip.ANI(p, 0)
    inp.x = inp.x + np.array([13.75, -7.25, 21.5])
    moved = ani2.compute(inp, ago=0, atom_virial=6)["atom_virial"]
    assert np.abs(moved - av).max() < 2 * ani.cutoffs()[0] * F_TOL * nmax
    ani.close()
    ani2.close()
