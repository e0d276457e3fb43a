"""The AEV stage alone against fp64, where the dispatch and the LDS capacities change (inputs and bars: tests/aev_edges.py,
proven without a GPU in tests/test_aev_edges_cpu.py).

Per case, ``radial_compat`` and path, one ``ANI.compute(inp, ago=0)`` and three comparisons:

* forward: the kernel's AEV rows, mapped to full width, against the fp64 oracle's; padding rows identically zero;
* backward: ``force`` (all ntotal rows) and ``virial`` against ``Oracle.aev_vjp`` run on the kernel's OWN dE/dAEV rows at full
  width, so a difference belongs to the backward kernel alone;
* the fp64 handle (``use_single=False``): forces against ``Oracle.compute`` within 1e-7 kcal/mol/A, the tolerance
  test_repulsion_term_rank_invariance_and_oracle uses, so that the ``aev64`` kernels meet the same edges.

The bars are min(margin x e32, cap) per quantity in the max norm (aev_edges.py, module docstring); the margin is
``aev_edges.MARGIN`` = 8 on every path (``MARGINS`` would hold a path whose margin had to be raised, with the reason; none had).

Paths (``PATHS``): the default options on the strong-last list, ``aev_fused`` 0, the same list with every segment shuffled; on
dense7-129, dense7-257 and shell-full also ``aev_symmetric_radial`` 0 and ``aev_tickets_min`` 0 (rows drawn by ticket); a half list
on dense7-193; ``vflag=False`` (the VIR = false instantiation) on dense7-129.

What the library documents and these tests assert where a capacity is exceeded:

* more than kMaxAng = 96 neighbours inside Rca: ANI_ERR_CAPACITY, the handle stays usable;
* more entries inside Rcr than radial_cap() with the radial screen on: the step is repeated once with the full capacity, the
  library says so on stderr, and the result meets the same bars (test_radial_capacity_overflow_is_retried_with_full_capacity);
* the generic kernels (``compact_neighbours``) and the fp64 kernels (``compact64``) hold kMaxRad = 256 radial entries per centre:
  one more raises the error flag, the step fails with ANI_ERR_CAPACITY (nothing is returned from a truncated list).  In compat
  mode every list entry is a radial entry, so a 257-entry list is refused there by the generic and by the fp64 kernels.

``ANI_AEV_EDGES_JSON=<file>`` writes the worst error / e32 of every (case, compat, path, quantity) with the margin in force
(profiles/aev_stage_edges.json is such a file).
"""
import functools
import json
import os

import numpy as np
import pytest

import aev_edges as ae
import stage_reference as sr
from lammps_ani_amd import ani_hip

pytestmark = pytest.mark.gpu

COMPAT = [False, True]
F64_TOL = 1e-7

# path -> (list form, options, vflag)
PATHS = {
    "fused1": ("strong-last", {}, True),
    "fused0": ("strong-last", dict(aev_fused=0), True),
    "shuffled": ("shuffled", {}, True),
    "symrad0": ("strong-last", dict(aev_symmetric_radial=0), True),
    "tickets0": ("strong-last", dict(aev_tickets_min=0), True),
    "half": ("half", {}, True),
    "novirial": ("strong-last", {}, False),
}
EXTRA = {"dense7-129": ("symrad0", "tickets0", "novirial"), "dense7-257": ("symrad0", "tickets0"), "shell-full": ("symrad0", "tickets0"),
         "dense7-193": ("half",)}
MARGINS = {}   # (case, path) -> a margin above aev_edges.MARGIN, never past the caps, with its reason next to it


def refused(name, compat, fp64=False):
    """kMaxRad = 256 radial entries per centre in the generic and the fp64 kernels; compat keeps every list entry"""
    c = ae.CASES[name]
    return compat and c.longest > ae.K_MAX_RAD and (fp64 or c.kernels == "generic")


RUNS = [(n, c, p) for n in ae.CASE_IDS for c in COMPAT for p in ("fused1", "fused0", "shuffled") + EXTRA.get(n, ()) if not refused(n, c)]
RUN_IDS = [f"{n}-{'compat' if c else 'strict'}-{p}" for n, c, p in RUNS]

RATIOS = {}    # "case/compat/path" -> dict(quantity -> worst error / e32, margin)
E32 = {}       # "case/compat" -> the e32 of each quantity (what the ratios are in units of)
FP64 = {}      # "case/compat" -> max |force of the fp64 handle - Oracle.compute|


@pytest.fixture(scope="module", autouse=True)
def _ratios():
    """after the module: the worst error / e32 of every run, on stdout (pytest -s) and into $ANI_AEV_EDGES_JSON"""
    yield
    for k in sorted(RATIOS):
        print("aev stage", k, " ".join(f"{q} {v:.3g}" for q, v in RATIOS[k].items()))
    out = os.environ.get("ANI_AEV_EDGES_JSON")
    if out and RATIOS:
        with open(out, "w") as f:
            json.dump(dict(unit="runs: worst |kernel - fp64 reference| / e32 (max norm) and the margin in force (bar = min(margin x e32, cap)); "
                                "e32: |fp32 oracle - fp64 oracle| per case (AEV units, kcal/mol/A, kcal/mol); "
                                "fp64_handle_force_error: kcal/mol/A against a tolerance of %g" % F64_TOL,
                           runs=RATIOS, e32=E32, fp64_handle_force_error=FP64), f, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def _oracle(path):
    from oracle import Oracle
    return Oracle(path)


def _input(name, form):
    return {"strong-last": ae.build_input, "shuffled": ae.shuffled, "half": ae.half_input}[form](name)


def _model_of(name):
    return ae.OVER[name]["model"] if name in ae.OVER else ae.CASES[name].model


def _step(ani, inp, vflag=True, ago=0):
    """one step and what the stage comparisons need: the result, the AEV rows at full width, the raw AEV array with the rows of
    the centres, and the kernel's dE/dAEV at full width"""
    out = ani.compute(inp, ago=ago, vflag=vflag)
    full, rows, v, _ = sr.full_width_rows(ani, inp.nlocal)
    raw = ani.debug_read(v.d_aev, (v.nrows, v.aev_stride), np.float32)
    return out, full, raw, rows, sr.full_width_gaev(ani, inp.nlocal)


def _check(tag, name, compat, path, inp, step, vflag=True, margin=None):
    """the forward and the backward comparison of one step against the references of ``name``; records and returns the ratios"""
    out, full, raw, rows, g = step
    ref = ae.reference(name, compat, path)
    bar = ae.bars(ref, margin if margin is not None else ae.MARGIN)
    pad = np.ones(raw.shape[0], bool)
    pad[rows] = False
    assert np.all(raw[pad] == 0), "padding rows of the AEV array are not zero"
    vjp = _oracle(path).aev_vjp(inp, g, radial_compat=compat)
    err = dict(aev=float(np.abs(full - ref["aev"]).max()), force=float(np.abs(out["force"] - vjp["force"]).max()))
    if vflag:
        err["virial"] = float(np.abs(out["virial"] - vjp["virial"]).max())
    ratio = {q: err[q] / ref["e32"][q] for q in err}
    print(tag, " ".join(f"{q}: err {err[q]:.3e} = {ratio[q]:.2f} e32 (bar {bar[q]:.2e}, cap {ref['cap'][q]:.2e})" for q in err))
    RATIOS[tag] = dict(ratio, margin=margin if margin is not None else ae.MARGIN)
    E32[f"{name}/{'compat' if compat else 'strict'}"] = ref["e32"]
    assert np.all(np.isfinite(out["force"]))
    for q in err:
        assert err[q] < bar[q], f"{tag} {q}: {err[q]:.3e} = {ratio[q]:.1f} e32, bar {bar[q]:.3e}"
    return ratio


@pytest.mark.parametrize("name,compat,path_id", RUNS, ids=RUN_IDS)
def test_aev_stage_against_fp64(name, compat, path_id, model_cache):
    form, opts, vflag = PATHS[path_id]
    inp = _input(name, form)
    assert inp.half or int(inp.numneigh.max()) == ae.CASES[name].longest or name == "degenerate"
    path = ae.model_path(ae.CASES[name].model, model_cache)
    ani = ani_hip.ANI(path, 0, -1, use_cuaev=not compat, use_fullnbr=not inp.half)
    for k, v in opts.items():
        ani.set_option(k, v)
    step = _step(ani, inp, vflag)
    ani.close()
    _check(f"{name}/{'compat' if compat else 'strict'}/{path_id}", name, compat, path, inp, step, vflag, MARGINS.get((name, path_id)))


@pytest.mark.parametrize("compat", COMPAT, ids=["strict", "compat"])
@pytest.mark.parametrize("name", ["dense7-257", "dense4-257"])
def test_past_256_both_aev_fused_settings_take_the_two_kernel_route(name, compat, model_cache):
    """launch_aev_forward_fused does not apply past 256 list entries: aev_fused 1 and 0 then run the same two kernels (compaction,
    forward), which sum in a fixed order -- the AEV arrays are equal bit for bit (each is held against fp64 above)"""
    inp = ae.build_input(name)
    path = ae.model_path(ae.CASES[name].model, model_cache)
    raws = []
    for fused in (1, 0):
        ani = ani_hip.ANI(path, 0, -1, use_cuaev=not compat)
        ani.set_option("aev_fused", fused)
        raws.append(_step(ani, inp)[2])
        ani.close()
    assert np.array_equal(raws[0], raws[1])


@pytest.mark.parametrize("compat", COMPAT, ids=["strict", "compat"])
@pytest.mark.parametrize("name", ae.CASE_IDS)
def test_fp64_handle_on_the_same_edges(name, compat, model_cache):
    inp = ae.build_input(name)
    path = ae.model_path(ae.CASES[name].model, model_cache)
    ani = ani_hip.ANI(path, 0, -1, use_cuaev=not compat, use_single=False)
    if refused(name, compat, fp64=True):
        with pytest.raises(ani_hip.AniError, match="capacity"):
            ani.compute(inp, ago=0)
        ani.close()
        return
    got = ani.compute(inp, ago=0)
    ani.close()
    ref = ae.reference(name, compat, path)
    err = float(np.abs(got["force"] - ref["force"]).max())
    print(f"{name} compat={int(compat)} fp64 handle: max|dF| {err:.2e}, |dE| {abs(got['energy'] - ref['energy']):.2e}")
    FP64[f"{name}/{'compat' if compat else 'strict'}"] = err
    assert err < F64_TOL


@pytest.mark.parametrize("name", [n for n in ae.CASE_IDS if refused(n, True)])
def test_generic_kernels_refuse_a_257th_radial_entry_in_compat_mode(name, model_cache):
    """compat keeps every list entry as a radial entry; the generic kernels hold kMaxRad = 256 per centre"""
    ani = ani_hip.ANI(ae.model_path(ae.CASES[name].model, model_cache), 0, -1, use_cuaev=False)
    with pytest.raises(ani_hip.AniError, match="capacity"):
        ani.compute(ae.build_input(name), ago=0)
    ani.close()


@pytest.mark.parametrize("compat", COMPAT, ids=["strict", "compat"])
@pytest.mark.parametrize("over,full", [("shell-angular-97", "shell-full"), ("generic-shell-radial-257", "generic-shell-full")])
def test_one_entry_past_a_hard_capacity_is_refused_and_the_handle_stays_usable(over, full, compat, model_cache):
    """97 neighbours inside Rca (kMaxAng = 96), or 257 inside Rcr in the generic kernels (kMaxRad = 256): ANI_ERR_CAPACITY; the
    same handle then computes the exactly-full cluster within the bars"""
    path = ae.model_path(_model_of(over), model_cache)
    ani = ani_hip.ANI(path, 0, -1, use_cuaev=not compat)
    with pytest.raises(ani_hip.AniError, match="capacity"):
        ani.compute(ae.build_input(over), ago=0)
    inp = ae.build_input(full)
    step = _step(ani, inp)
    ani.close()
    _check(f"{full}/{'compat' if compat else 'strict'}/after-{over}", full, compat, path, inp, step)


def test_one_entry_past_the_screened_radial_capacity_is_retried_with_the_full_one(model_cache, capfd):
    """193 entries inside Rcr against radial_cap(256) = 192, 96 inside Rca: the step is repeated with the capacity of the full
    list, the library says so once, and the result meets the bars of the stage (both from the repeated step and from the next)"""
    name = "shell-radial-193"
    path = ae.model_path(_model_of(name), model_cache)
    inp = ae.build_input(name)
    ani = ani_hip.ANI(path, 0)
    step = _step(ani, inp)
    assert "full_radial_capacity = 1" in capfd.readouterr().err
    _check(f"{name}/strict/retried", name, False, path, inp, step)
    again = _step(ani, inp, ago=1)
    assert "full_radial_capacity" not in capfd.readouterr().err
    _check(f"{name}/strict/after-retry", name, False, path, inp, again)
    ani.close()
    # compat: the capacity is the list length, nothing overflows
    ani = ani_hip.ANI(path, 0, -1, use_cuaev=False)
    step = _step(ani, inp)
    assert "full_radial_capacity" not in capfd.readouterr().err
    ani.close()
    _check(f"{name}/compat/fused1", name, True, path, inp, step)
