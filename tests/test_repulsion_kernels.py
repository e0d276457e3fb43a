"""GPU: the pairwise repulsion ALONE (null networks) on every kernel path, against the numpy fp64 pair sums of
tests/repulsion_reference.py under that module's derived bars.

Paths, each asserted through ``ani_last_repulsion_kernel``:
  aev_backward_fast          folded into the fast AEV backward kernel (fp32, at most 8 species present, block cutoff <= Rcr or pyaev)
  repulsion_kernel<float>    the stand-alone kernel beside the generic AEV backward, and for a block cutoff beyond Rcr
  repulsion_kernel<double>   the fp64 handle
and the armed (per-atom virial) instantiation of each.  tests/test_repulsion_reference_cpu.py shows that the reference is the
oracle's repulsion to 1e-10 and that each of the reference's mutations (pairs beyond Rcr dropped, tables by compact species, a
wrong k_rep, no cutoff derivative, ghosts whole, the energy's half) moves some output of every case by at least ten bars.
The bars are min(MARGIN x first-order model, cap); see the reference's docstring.  Worst error / bar per case: the module's report.
"""
import numpy as np
import pytest

import repulsion_reference as rr
from lammps_ani_amd import model_file as mf

pytestmark = pytest.mark.gpu

FOLDED, ALONE32, ALONE64 = "aev_backward_fast", "repulsion_kernel<float>", "repulsion_kernel<double>"
WORST = {}


@pytest.fixture(scope="module")
def hip():
    from lammps_ani_amd import ani_hip
    return ani_hip


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    """after the module: the worst error / bar of each case and output, on stdout (pytest -s shows it)"""
    yield
    for k in sorted(WORST):
        print(f"repulsion {k:>28s}: " + "  ".join(f"{q} {v:.3g}" for q, v in WORST[k].items()))


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    d = tmp_path_factory.mktemp("null_models")
    cache = {}

    def get(case, repulsion=True):
        key = (case, repulsion)
        if key not in cache:
            p = str(d / f"{case}{'' if repulsion else '_noblock'}.anim")
            mf.write_model(p, rr.case_model(case, repulsion))
            cache[key] = p
        return cache[key]

    return get


def _check(tag, got, inp, ref, bar, expected, kernel, ncomp=0):
    """force (owned and ghost rows), energy, virial, optionally the per-atom virial against the reference under ``bar``"""
    assert kernel == expected, (tag, kernel)
    assert np.all(np.isfinite(got["force"])) and np.isfinite(got["energy"])
    w = dict(force=float(rr.ratio(np.abs(got["force"] - ref["force"]).max(1), bar["force"]).max()),
             energy=abs(got["energy"] - ref["energy"]) / bar["energy"],
             virial=float(np.abs(got["virial"] - ref["virial"]).max()) / bar["virial"])
    if ncomp:
        assert got["atom_virial"].shape == (inp.ntotal, ncomp)
        w[f"atom_virial{ncomp}"] = float(rr.ratio(np.abs(got["atom_virial"] - ref["atom_virial"](ncomp)).max(1), bar["atom_virial"]).max())
    print(f"{tag} [{kernel}]: error / bar " + " ".join(f"{q} {v:.3g}" for q, v in w.items())
          + f"; |dF| {np.abs(got['force'] - ref['force']).max():.2e} |dE| {abs(got['energy'] - ref['energy']):.2e}"
          + f" |dV| {np.abs(got['virial'] - ref['virial']).max():.2e}")
    WORST[tag] = w
    assert np.all(got["eatom"] == 0.0)     # the repulsion is not part of eatom
    for q, v in w.items():
        assert v <= 1.0, f"{tag} {q}: error / bar {v:.3g}"


def _run(hip, path, inp, single=True, cuaev=True, opts=(), ncomp=0):
    ani = hip.ANI(path, 0, -1, use_cuaev=cuaev, use_single=single)
    for k, v in opts:
        ani.set_option(k, v)
    got = ani.compute(inp, ago=0, atom_virial=ncomp)
    kernel = ani.last_repulsion_kernel()
    ani.close()
    return got, kernel


@pytest.mark.parametrize("case,single", [("mixed64", True), ("tiny64", True), ("mixed64", False)],
                         ids=["folded-shape", "generic-shape", "double"])
def test_null_network_without_the_block_is_exactly_zero(case, single, model_path, hip):
    """The isolation, proved: on each of the three paths a null model WITHOUT the block gives exact zeros everywhere."""
    inp = rr.case_input(case)
    ani = hip.ANI(model_path(case, False), 0, -1, use_single=single)
    assert ani.last_repulsion_kernel() == ""
    got = ani.compute(inp, ago=0)
    assert ani.last_repulsion_kernel() == ""
    ani.close()
    assert np.all(got["force"] == 0.0) and got["energy"] == 0.0 and np.all(got["eatom"] == 0.0) and np.all(got["virial"] == 0.0)


# id: (case, use_single, use_cuaev, options, expected kernel)
RUNS = {
    "mixed64": ("mixed64", True, True, (), FOLDED),
    "mixed64-nosym": ("mixed64", True, True, (("aev_symmetric_radial", 0),), FOLDED),
    "mixed64-pyaev": ("mixed64", True, False, (), FOLDED),
    "mixed64-cut51": ("mixed64-cut51", True, True, (), FOLDED),
    "water-HO-tables1": ("water-HO", True, True, (("aev_stream_tables", 1),), FOLDED),
    "water-HO-tables0": ("water-HO", True, True, (("aev_stream_tables", 0),), FOLDED),
    "seven": ("seven", True, True, (), FOLDED),
    "tiny64": ("tiny64", True, True, (), ALONE32),
    "open40-ani1x": ("open40-ani1x", True, True, (), FOLDED),
    "open40-tiny": ("open40-tiny", True, True, (), ALONE32),
    "double-mixed64": ("mixed64", False, True, (), ALONE64),
    "double-tiny64": ("tiny64", False, True, (), ALONE64),
    "soft-cut60": ("soft-cut60", True, True, (), ALONE32),
    "soft-cut60-double": ("soft-cut60", False, True, (), ALONE64),
    "soft-cut60-pyaev": ("soft-cut60", True, False, (), FOLDED),     # every candidate is live: the folded path sees the pairs beyond Rcr
}


@pytest.mark.parametrize("run", list(RUNS))
def test_repulsion_alone_matches_the_pair_sum(run, model_path, hip):
    case, single, cuaev, opts, expected = RUNS[run]
    inp, m, ref, b32, b64 = rr.case_reference(case)
    got, kernel = _run(hip, model_path(case), inp, single, cuaev, opts)
    _check(run, got, inp, ref, b32 if single else b64, expected, kernel)


@pytest.mark.parametrize("ncomp", [9, 6])
@pytest.mark.parametrize("case,single,expected", [("mixed64", True, FOLDED), ("tiny64", True, ALONE32), ("mixed64", False, ALONE64)],
                         ids=["folded", "alone32", "alone64"])
def test_armed_instantiations(case, single, expected, ncomp, model_path, hip):
    """the per-atom virial of the three armed instantiations, with the step's other outputs"""
    inp, m, ref, b32, b64 = rr.case_reference(case)
    got, kernel = _run(hip, model_path(case), inp, single, ncomp=ncomp)
    _check(f"armed-{case}-{'fp32' if single else 'fp64'}-{ncomp}", got, inp, ref, b32 if single else b64, expected, kernel, ncomp)


def test_split_step(model_path, hip):
    """mixed64 through ani_step_begin / ani_step_ghosts_ready / ani_step_finish (driven as tests/test_split_step.py does): two row
    ranges, no symmetric collection, one energy"""
    import torch
    dev = torch.device("cuda:0")
    inp, m, ref, b32, _ = rr.case_reference("mixed64")
    nt, nl = inp.ntotal, inp.nlocal
    d = dict(x=torch.from_numpy(inp.x.reshape(-1).copy()).to(dev), species=torch.from_numpy(inp.species.astype(np.int32)).to(dev),
             ilist=torch.from_numpy(inp.ilist).to(dev), numneigh=torch.from_numpy(inp.numneigh).to(dev),
             jlist=torch.from_numpy(inp.jlist).to(dev))
    ani = hip.ANI(model_path("mixed64"), 0, -1)
    ani.set_option("device_overwrite_forces", 1)
    f = torch.zeros(nt * 3, dtype=torch.float64, device=dev)
    ev = torch.zeros(10, dtype=torch.float64, device=dev)
    ea = torch.zeros(nl, dtype=torch.float64, device=dev)
    ani.compute_device(nt, nl, d["species"].data_ptr(), d["x"].data_ptr(), inp.npairs, d["ilist"].data_ptr(), d["jlist"].data_ptr(),
                       d["numneigh"].data_ptr(), 0, f.data_ptr(), ev.data_ptr(), ea.data_ptr(), eflag_atom=True, vflag=True)
    torch.cuda.synchronize()
    f.fill_(float("nan"))
    ev.fill_(float("nan"))
    ani.step_begin(nt, nl, d["x"].data_ptr(), f.data_ptr(), ev.data_ptr(), ea.data_ptr(), eflag_atom=True, vflag=True)
    ani.step_ghosts_ready()
    ani.step_finish()
    torch.cuda.synchronize()
    evh = ev.cpu().numpy()
    got = dict(force=f.cpu().numpy().reshape(nt, 3), energy=float(evh[0]), virial=evh[1:10].reshape(3, 3), eatom=ea.cpu().numpy())
    kernel = ani.last_repulsion_kernel()
    ani.close()
    _check("split-mixed64", got, inp, ref, b32, FOLDED, kernel)


def test_two_bricks(model_path, hip):
    """mixed64 as (2, 1, 1): each rank against its own reference (half share of the owned-ghost pairs); the two device energies
    sum to the one-rank reference within the sum of the ranks' bars"""
    one = rr.case_reference("mixed64")[2]["energy"]
    total, tol = 0.0, 0.0
    for rank in (0, 1):
        inp, m, ref, b32, _ = rr.case_reference("mixed64", (2, 1, 1), rank)
        got, kernel = _run(hip, model_path("mixed64"), inp)
        _check(f"bricks-rank{rank}", got, inp, ref, b32, FOLDED, kernel)
        total += got["energy"]
        tol += b32["energy"]
    assert abs(total - one) <= tol


@pytest.mark.parametrize("case,expected", [("mixed64", FOLDED), ("tiny64", ALONE32)])
def test_second_step_on_the_cached_list(case, expected, model_path, hip):
    """ago = 1: the erep slots are cleared per step, not accumulated -- the second energy is the first (one add per slot and a
    fixed tree: to the fp64 bar of the case, 4e-14 of the energy) and still the reference's"""
    inp, m, ref, b32, b64 = rr.case_reference(case)
    ani = hip.ANI(model_path(case), 0, -1)
    first = ani.compute(inp, ago=0)
    second = ani.compute(inp, ago=1)
    kernel = ani.last_repulsion_kernel()
    ani.close()
    assert abs(second["energy"] - first["energy"]) <= b64["energy"]
    _check(f"reuse-{case}", second, inp, ref, b32, expected, kernel)
