"""GPU: the neighbour-list contract of include/ani_hip.h with an ilist that is NOT the identity, at the edges of the rebuild-time
code.

The header: ``ilist_unique[nlocal]`` is an arbitrary ordering of the owned atoms; ``numneigh[ii]`` and the jlist segments follow ilist
order; ``out_atomic_energies`` and ``atom_energy_dev`` come back in ilist order; forces, the per-atom virial, ``member_dforce`` and
``atom_force_dev`` by atom.  Every kernel that carries both the atom index i and the centre position ii (prepare_count_kernel,
prepare_rows_kernel with row_info = {i, off, len, ii}, row_of_atom[i], centre_of_row[row] = ii, species[ilist[ii]] in the finish
kernels, the symmetric radial collection, list_symmetry_kernel, the row classes of the split step) could mix the two and stay
unnoticed by an identity ilist, which is all the harness, the golden fixtures and the device list builders ever produce.

Inputs and forms come from tests/list_forms.py; tests/test_list_forms_cpu.py shows on the fp64 oracle that a form changes a result
only by ``expected()`` (1e-13 on forces), so one oracle result per input serves every form.  The oracle (oracle/ani_oracle.c) walks
ilist itself and is the independent reference, also above the 4096 centres of one preparation / scan chunk.

Bars, none of them made here:
  against the oracle, fp32   tests/test_hip_parity.py ``_check``: E 2e-3 * max(1, n/100), F 2.3e-3, eatom 2e-3, V 2e-2 * max(1, n/100)
  against the oracle, fp64   test_hip_double_precision_matches_golden: F 1e-8, eatom 1e-7, V 1e-6, E 9e-9 relative
  form against identity run  tests/test_split_step.py, "same arithmetic, fp32 atomics in another order": F 2e-4 + 2e-6 max|F|,
                             E 1e-3 * max(1, nl/1000), eatom 1e-4, V 1e-5 max|V| + 1e-2
"""
import dataclasses

import numpy as np
import pytest

import list_forms as lf
from test_hip_parity import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from lammps_ani_amd import ani_hip
    return ani_hip


@pytest.fixture(scope="module")
def oracle_ref(model_cache):
    """(input id, radial_compat) -> oracle result of the identity form, computed once and never modified"""
    from oracle import Oracle
    cache = {}

    def get(name, compat=False):
        if (name, compat) not in cache:
            cache[(name, compat)] = Oracle(lf.model_path(name, model_cache)).compute(lf.build_input(name), radial_compat=compat)
        return cache[(name, compat)]

    return get


def _reorder_bars(ref_run, nl):
    fmax = float(np.abs(ref_run["force"]).max())
    vmax = float(np.abs(ref_run["virial"]).max())
    return dict(force=2e-4 + 2e-6 * fmax, energy=1e-3 * max(1.0, nl / 1000.0), eatom=1e-4, virial=1e-5 * vmax + 1e-2)


def _check_reorder(got, want, bars, label):
    de = abs(got["energy"] - want["energy"])
    df = float(np.abs(got["force"] - want["force"]).max())
    dea = float(np.abs(got["eatom"] - want["eatom"]).max())
    dv = float(np.abs(got["virial"] - want["virial"]).max())
    print(f"{label}: |dE|={de:.2e} (bar {bars['energy']:.1e}) max|dF|={df:.2e} (bar {bars['force']:.1e}) "
          f"max|dEatom|={dea:.2e} (bar {bars['eatom']:.1e}) max|dV|={dv:.2e} (bar {bars['virial']:.1e})")
    assert de < bars["energy"]
    assert df < bars["force"]
    assert dea < bars["eatom"]
    assert dv < bars["virial"]


def _check64(got, ref, label):
    de = abs(got["energy"] - ref["energy"])
    print(f"{label}: |dE|={de:.2e} (|E|={abs(ref['energy']):.2e}) max|dF|={np.abs(got['force'] - ref['force']).max():.2e} "
          f"max|dEatom|={np.abs(got['eatom'] - ref['eatom']).max():.2e} max|dV|={np.abs(got['virial'] - ref['virial']).max():.2e}")
    assert de < 9e-9 * abs(ref["energy"])
    np.testing.assert_allclose(got["force"], ref["force"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(got["eatom"], ref["eatom"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(got["virial"], ref["virial"], rtol=0, atol=1e-6)


def _moved(inp, seed=0):
    """the same input with every position perturbed by normal(0, 0.02) (ghosts move independently: fine for a parity check)"""
    return dataclasses.replace(inp, x=inp.x + np.random.default_rng(seed).normal(0, 0.02, size=inp.x.shape))


HOST_CASES = [(n, "strict") for n in lf.INPUT_IDS] + [("mixed7_brick", "compat")]


# ---- 1. host entry against the oracle ---------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["reversed", "random+shuffled"])
@pytest.mark.parametrize("name,mode", HOST_CASES, ids=[f"{n}-{m}" for n, m in HOST_CASES])
def test_host_entry_matches_oracle_in_every_form(name, mode, form, model_cache, hip, oracle_ref):
    from oracle import Oracle
    compat = mode == "compat"
    p = lf.model_path(name, model_cache)
    base = lf.build_input(name)
    inp, perm = lf.apply_form(base, form)
    ani = hip.ANI(p, 0, use_cuaev=not compat)
    got = ani.compute(inp, ago=0)
    _check(got, lf.expected(oracle_ref(name, compat), perm), inp.nlocal, f"{name}/{mode}/{form}/ago=0")
    # the cached permuted list with new positions
    moved = _moved(inp)
    ref1 = Oracle(p).compute(dataclasses.replace(base, x=moved.x), radial_compat=compat)
    got1 = ani.compute(moved, ago=1)
    _check(got1, lf.expected(ref1, perm), inp.nlocal, f"{name}/{mode}/{form}/ago=1")
    ani.close()


# ---- 2. reordering the centres changes only the order of the fp32 atomics -----------------------------------------------

@pytest.mark.parametrize("name", lf.INPUT_IDS)
def test_reordered_centres_equal_the_identity_run(name, model_cache, hip):
    """``reversed`` and ``random`` keep every segment's order, so every AEV row and network output is the same arithmetic as in
    the identity run; only the rows' places in the buckets and the order of the force atomics differ."""
    base = lf.build_input(name)
    ani = hip.ANI(lf.model_path(name, model_cache), 0)
    ident = ani.compute(base, ago=0)
    bars = _reorder_bars(ident, base.nlocal)
    for form in ("reversed", "random"):
        inp, perm = lf.apply_form(base, form)
        _check_reorder(ani.compute(inp, ago=0), lf.expected(ident, perm), bars, f"{name}/{form} vs identity run")
    ani.close()


# ---- 3. double precision ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["chunk4097", "ghost_only_species", "tiny_generic"])
def test_double_precision_matches_oracle(name, model_cache, hip, oracle_ref):
    inp, perm = lf.apply_form(lf.build_input(name), "random+shuffled")
    ani = hip.ANI(lf.model_path(name, model_cache), 0, use_single=False)
    for ago in (0, 1):
        _check64(ani.compute(inp, ago=ago), lf.expected(oracle_ref(name), perm), f"{name}/double/ago={ago}")
    ani.close()


# ---- 4. options that change who handles a row -------------------------------------------------------------------------

@pytest.mark.parametrize("option", ["aev_symmetric_radial", "aev_fused", "aev_tickets_min", "mlp_fused"])
@pytest.mark.parametrize("name", ["chunk4097", "mixed7_brick"])
def test_row_handling_options_match_oracle(name, option, model_cache, hip, oracle_ref):
    inp, perm = lf.apply_form(lf.build_input(name), "random")
    ani = hip.ANI(lf.model_path(name, model_cache), 0)
    ani.set_option(option, 0)
    want = lf.expected(oracle_ref(name), perm)
    for ago in (0, 1):
        _check(ani.compute(inp, ago=ago), want, inp.nlocal, f"{name}/{option}=0/ago={ago}")
    ani.close()


# ---- 5. device entry and split step ------------------------------------------------------------------------------------

def _device_arrays(inp, dev):
    import torch
    return dict(x=torch.from_numpy(inp.x.reshape(-1).copy()).to(dev), species=torch.from_numpy(inp.species.astype(np.int32)).to(dev),
                ilist=torch.from_numpy(inp.ilist.copy()).to(dev), numneigh=torch.from_numpy(inp.numneigh.copy()).to(dev),
                jlist=torch.from_numpy(inp.jlist.copy()).to(dev))


def _device_result(f, ev, ea):
    return dict(energy=float(ev[0]), force=f.view(-1, 3).cpu().numpy(), eatom=ea.cpu().numpy(), virial=ev[1:].cpu().numpy().reshape(3, 3))


@pytest.mark.parametrize("name", ["chunk4097", "mixed7_brick"])
def test_device_entry_and_split_step_match_oracle(name, model_cache, hip, oracle_ref):
    import torch
    dev = torch.device("cuda:0")
    inp, perm = lf.apply_form(lf.build_input(name), "random")
    want = lf.expected(oracle_ref(name), perm)
    nt, nl = inp.ntotal, inp.nlocal
    d = _device_arrays(inp, dev)
    ani = hip.ANI(lf.model_path(name, model_cache), 0)
    ani.set_option("device_overwrite_forces", 1)

    def outputs():
        return (torch.full((nt * 3,), float("nan"), dtype=torch.float64, device=dev),
                torch.full((10,), float("nan"), dtype=torch.float64, device=dev),
                torch.full((nl,), float("nan"), dtype=torch.float64, device=dev))

    f, ev, ea = outputs()
    ani.compute_device(nt, nl, d["species"].data_ptr(), d["x"].data_ptr(), inp.npairs, d["ilist"].data_ptr(), d["jlist"].data_ptr(),
                       d["numneigh"].data_ptr(), 0, f.data_ptr(), ev.data_ptr(), ea.data_ptr(), eflag_atom=True, vflag=True)
    torch.cuda.synchronize()
    _check(_device_result(f, ev, ea), want, nl, f"{name}/random/compute_device")   # d_eatom in ilist order
    for rep in range(2):   # the second split step reuses the row classes of the epoch
        x = d["x"].clone()
        ghosts = x[3 * nl:].clone()
        x[3 * nl:] = float("nan")                    # part 1 must not read a ghost position
        f, ev, ea = outputs()
        ani.step_begin(nt, nl, x.data_ptr(), f.data_ptr(), ev.data_ptr(), ea.data_ptr(), eflag_atom=True, vflag=True)
        torch.cuda.synchronize()
        x[3 * nl:] = ghosts
        ani.step_ghosts_ready()
        torch.cuda.synchronize()
        ani.step_finish()
        torch.cuda.synchronize()
        _check(_device_result(f, ev, ea), want, nl, f"{name}/random/split step {rep}")
    ani.close()


def test_device_entry_with_a_ghost_free_fold(model_cache, hip, oracle_ref):
    """cluster_isolated has no ghosts: ani_set_ghost_fold accepts nghost == 0 (maps of length zero), and the folded step is the
    plain one.  Zero-length rows between dense ones, through the device entry."""
    import torch
    dev = torch.device("cuda:0")
    name = "cluster_isolated"
    inp, perm = lf.apply_form(lf.build_input(name), "random")
    want = lf.expected(oracle_ref(name), perm)
    nt, nl = inp.ntotal, inp.nlocal
    assert nt == nl
    d = _device_arrays(inp, dev)
    owner = torch.zeros(1, dtype=torch.int64, device=dev)     # never read: nghost is 0
    shift = torch.zeros(3, dtype=torch.float64, device=dev)
    ani = hip.ANI(lf.model_path(name, model_cache), 0)
    ani.set_option("device_overwrite_forces", 1)
    for ago in (0, 1):
        f = torch.full((nt * 3,), float("nan"), dtype=torch.float64, device=dev)
        ev = torch.full((10,), float("nan"), dtype=torch.float64, device=dev)
        ea = torch.full((nl,), float("nan"), dtype=torch.float64, device=dev)
        ani.compute_device(nt, nl, d["species"].data_ptr(), d["x"].data_ptr(), inp.npairs, d["ilist"].data_ptr(), d["jlist"].data_ptr(),
                           d["numneigh"].data_ptr(), ago, f.data_ptr(), ev.data_ptr(), ea.data_ptr(), eflag_atom=True, vflag=True)
        torch.cuda.synchronize()
        got = _device_result(f, ev, ea)
        _check(got, want, nl, f"{name}/random/compute_device ago={ago}{' folded' if ago else ''}")
        isolated = np.flatnonzero(inp.numneigh == 0)
        assert len(isolated) >= lf.N_ISOLATED and np.all(got["force"][inp.ilist[isolated]] == 0)
        if ago == 0:
            ani.set_ghost_fold(owner.data_ptr(), shift.data_ptr(), 0)
    ani.close()


# ---- 6. armed steps ---------------------------------------------------------------------------------------------------

def test_armed_step_outputs_follow_the_header(model_cache, hip):
    """atom virial by atom, atom_energy_dev by centre, atom_force_dev / member_dforce by atom: a randomly ordered ilist against
    ``expected()`` of the identity run of the same handle (whose own correctness tests/test_atom_virial.py and
    tests/test_model_deviation.py cover)."""
    name = "cluster_isolated"
    base = lf.build_input(name)
    inp, perm = lf.apply_form(base, "random")
    nl = base.nlocal
    ani = hip.ANI(lf.model_path(name, model_cache), 0)
    ident = ani.compute(base, ago=0, atom_virial=9, deviation=True)
    got = ani.compute(inp, ago=0, atom_virial=9, deviation=True)
    want = lf.expected(ident, perm)
    bars = _reorder_bars(ident, nl)
    _check_reorder(got, want, bars, f"{name}/random armed vs identity run")
    av_bar = 1e-5 * float(np.abs(ident["atom_virial"]).max()) + 1e-2   # the virial bar on the per-atom entries
    dav = float(np.abs(got["atom_virial"] - want["atom_virial"]).max())
    gd, wd = got["deviation"], want["deviation"]
    dme = float(np.abs(gd["member_energy"] - wd["member_energy"]).max())
    dsig = float(np.abs(gd["atom_energy_dev"] - wd["atom_energy_dev"]).max())
    ddf = float(np.abs(gd["member_dforce"] - wd["member_dforce"]).max())
    dfd = float(np.abs(gd["atom_force_dev"] - wd["atom_force_dev"]).max())
    dsum = np.abs(gd["summary"] - wd["summary"])
    print(f"{name}/random armed: max|dW|={dav:.2e} (bar {av_bar:.1e}) |dE_m|={dme:.2e} max|dsigma_E|={dsig:.2e} max|d dF_m|={ddf:.2e} "
          f"max|d d_j|={dfd:.2e} summary {dsum}")
    assert dav < av_bar
    assert dme < bars["energy"]
    assert dsig < bars["eatom"]
    assert ddf < bars["force"]
    assert dfd < bars["force"]
    assert dsum[0] < bars["force"] and dsum[1] < bars["force"] and dsum[2] < nl * bars["force"] and dsum[3] < bars["eatom"]
    # the discriminating power of the comparison: by-centre outputs in atom order would miss by far more than the bar
    assert np.abs(ident["deviation"]["atom_energy_dev"] - want["deviation"]["atom_energy_dev"]).max() > 1000 * bars["eatom"]
    ani.close()


# ---- 7. device-built list across scan chunks ----------------------------------------------------------------------------

def _sorted_segments(nn, jl):
    """every segment sorted, flattened (one lexsort: the key is (centre, neighbour))"""
    centre = np.repeat(np.arange(len(nn)), nn)
    return jl[np.lexsort((jl, centre))]


@pytest.mark.parametrize("rows", [1, 0], ids=["sorted_rows", "count_then_fill"])
def test_device_built_list_across_scan_chunks(rows, model_cache, hip):
    """8193 centres: the neighbour-count scan (scan_chunk_kernel / scan_add_kernel, 4096 per chunk) adds two chunk totals in front
    of the third chunk; the second build has a row capacity.  Integer work: exact."""
    import torch
    dev = torch.device("cuda:0")
    inp = lf.build_input("chunk8193")
    ani = hip.ANI(lf.model_path("chunk8193", model_cache), 0)
    ani.set_option("nbr_sorted_rows", rows)
    x = torch.as_tensor(inp.x, dtype=torch.float64, device=dev).contiguous()
    sp = torch.as_tensor(inp.species.astype(np.int32), device=dev)
    lo, hi = inp.x.min(0) - 0.25, inp.x.max(0) + 0.25
    want = _sorted_segments(inp.numneigh, inp.jlist)
    for build in range(2):
        n = ani.build_list_device(inp.ntotal, inp.nlocal, sp.data_ptr(), x.data_ptr(), 7.1, lo, hi)
        torch.cuda.synchronize()
        assert n == inp.npairs
        nn, jl = ani.debug_list(inp.nlocal)
        assert np.array_equal(nn, inp.numneigh), (rows, build)
        assert np.array_equal(_sorted_segments(nn, jl), want), (rows, build)
    ani.close()
