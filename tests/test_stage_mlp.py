"""The MLP stage alone against fp64, at the row-tile edges, in every form the options reach; and its repeatability.

The reference (tests/stage_reference.py) runs the ensemble in numpy fp64 on the kernel's OWN AEV rows, so what is compared
is the MLP kernels alone: every real row's dE/dAEV (``d_gaev``) and every atom's energy, under bars derived from the
arithmetic of each form (module docstring of stage_reference.py).

Boxes: species buckets are padded to 128 rows and the kernels tile them by 16, 32, 64 and 128 rows, so the per-species atom
counts sit on those edges (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257), given explicitly.

Forms (option values -> the kernel ``last_mlp_kernel()`` must name; P = 3 for mlp_arith 1, 2 for mlp_arith 2):

    form id             mlp_fused  gen  rows  halves  schedule  chain   kernel
    default                 1       1     0     1        1        1     mlp_fused16<P, 4 or 8> (mlp_chain for gen 0, M = 1, small)
    m2-g1-r128-h0           2       1   128     0        1        1     mlp_fused16<P, 8>
    m2-g1-r128-h2           2       1   128     2        1        1     mlp_fused16<P, 8>   (every item as two halves)
    m2-g1-r64-h1            2       1    64     1        1        1     mlp_fused16<P, 4>
    m2-g1-r64-h2            2       1    64     2        1        1     mlp_fused16<P, 4>
    m2-g1-r128-sched0       2       1   128     1        0        1     mlp_fused16<P, 8>   (a work counter, no static schedule)
    m3-g1-r128-h1           3       1   128     1        1        1     mlp_fused16<P, 8>   (members in sequence)
    m2-g0                   2       0     -     -        1        1     mlp_fused<P>
    m3-g0                   3       0     -     -        1        1     mlp_fused<P>
    m0-chain0               0       -     -     -        -        0     gemm_grouped (one launch per layer)
    m0-chain1               0       -     -     -        -        1     mlp_chain (one member, small) else gemm_grouped

``mlp_arith`` 0 (fp32 products) has no fused kernel: it runs with the per-layer forms.  ``mlp_pipeline`` 1 and 2 are out of
scope (an opt-in with a known race and a test of its own).

Padding rows: a row of a species bucket past its last atom has ``centre_of_row = -1``; every kernel seeds its backward pass
with 0 there, so a padding row that the kernel processes gets dE/dAEV = 0 exactly.  The sixteen-row kernel skips work items
that hold no real row (64-row items, 32-row half items), whose rows are neither written nor read (the AEV backward reads
rows through ``row_of_centre`` only).  To make both halves of that contract observable, every case runs a first step,
fills the whole dE/dAEV array with NaN bytes, and runs the step again on the cached list: asserted are real rows contiguous
per species, the padding rows inside the first item-sized block after a bucket's last atom exactly zero (rewritten, not
left over), and the second step's energies equal to the first's bit for bit and its forces finite and equal to the first's
to the order of the force atomics (whatever stays NaN is never read).
"""
import ctypes
import hashlib

import numpy as np
import pytest

import stage_reference as sr
from lammps_ani_amd import ani_hip, harness as hx, model_file as mf

pytestmark = pytest.mark.gpu

WORST = {}   # (form id, arith) -> worst error / bar seen


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    """after the module: the worst error / bar of each form, on stdout (pytest -s shows it)"""
    yield
    for k in sorted(WORST):
        print(f"mlp stage {k[0]:>20s} arith {k[1]}: worst error / bar {WORST[k]:.3g}")


def _system(counts, spacing=1.6, seed=0):
    """Atoms on a jittered simple-cubic lattice in an open box, species counts as given (types 1..len(counts)), shuffled."""
    n = int(sum(counts))
    side = int(np.ceil(n ** (1 / 3)))
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(np.float64)
    x = g * spacing + rng.uniform(-0.2, 0.2, size=(n, 3))
    types = np.concatenate([np.full(c, t + 1, np.int32) for t, c in enumerate(counts)])
    types = types[rng.permutation(n)]
    L = side * spacing + 40.0
    return hx.System(x - x.mean(0), types, np.full(3, -L / 2), np.full(3, L / 2), periodic=(False, False, False))


# box id -> (model kind, members, species counts)
BOXES = {
    "ani2x-m8-all7": ("ani2x", 8, [129, 15, 1, 64, 33, 127, 17]),        # 1008 columns (63 k-steps of 16: odd)
    "ani2x-m2-absent": ("ani2x", 2, [257, 31, 0, 128, 65, 16, 63]),      # one species absent: columns pruned
    "ani1x-m1": ("ani1x", 1, [255, 32, 256, 1]),                          # 384 columns
    "ani2x-m2-five": ("ani2x", 2, [63, 129, 17, 31, 128, 0, 0]),         # the 560-column five-species shape
    "ani2x-m1-one-atom": ("ani2x", 1, [0, 0, 0, 1]),
}
_INPUTS = {}


def _input(box):
    if box not in _INPUTS:
        if box == "water-50001-m1":
            _INPUTS[box] = hx.decompose(hx.water_box(50001, seed=8))
        else:
            _INPUTS[box] = hx.decompose(_system(BOXES[box][2], seed=len(box)))
    return _INPUTS[box]


def _model(box, model_cache):
    kind, nm = ("ani2x", 1) if box == "water-50001-m1" else BOXES[box][:2]
    return model_cache(kind, nm, 41)


G = dict(mlp_fused_gen=1)
FORMS = {
    "default": dict(),
    "m2-g1-r128-h0": dict(mlp_fused=2, mlp_fused_rows=128, mlp_fused_halves=0, **G),
    "m2-g1-r128-h2": dict(mlp_fused=2, mlp_fused_rows=128, mlp_fused_halves=2, **G),
    "m2-g1-r64-h1": dict(mlp_fused=2, mlp_fused_rows=64, mlp_fused_halves=1, **G),
    "m2-g1-r64-h2": dict(mlp_fused=2, mlp_fused_rows=64, mlp_fused_halves=2, **G),
    "m2-g1-r128-sched0": dict(mlp_fused=2, mlp_fused_rows=128, mlp_fused_schedule=0, **G),
    "m3-g1-r128-h1": dict(mlp_fused=3, mlp_fused_rows=128, mlp_fused_halves=1, **G),
    "m2-g0": dict(mlp_fused=2, mlp_fused_gen=0),
    "m3-g0": dict(mlp_fused=3, mlp_fused_gen=0),
    "m0-chain0": dict(mlp_fused=0, mlp_chain=0),
    "m0-chain1": dict(mlp_fused=0, mlp_chain=1),
}
FUSED = [f for f in FORMS if f.startswith(("m2", "m3"))]


def _expected_kernel(form, arith, nm, nlocal):
    P = 3 if arith == 1 else 2
    o = FORMS[form]
    if arith == 0 or o.get("mlp_fused", 1) == 0:
        if form == "m0-chain1" and nm == 1 and arith != 0 and nlocal < 30000:
            return ("mlp_chain",)
        if form == "m0-chain1" and nm == 1 and arith != 0:
            return ("mlp_chain", "gemm_grouped")
        return ("gemm_grouped",)
    if o.get("mlp_fused_gen", 1) == 0:
        return ("mlp_fused<%d>" % P,)
    rows = o.get("mlp_fused_rows", 0)
    if rows == 128:
        return ("mlp_fused16<%d, 8>" % P,)
    if rows == 64:
        return ("mlp_fused16<%d, 4>" % P,)
    return ("mlp_fused16<%d, 8>" % P, "mlp_fused16<%d, 4>" % P)


_HIP = None


def _poison(d_ptr, nbytes):
    """fill a device buffer of the handle with 0xFF bytes (a NaN in every float), synchronously"""
    global _HIP
    if _HIP is None:
        _HIP = ctypes.CDLL("libamdhip64.so")
        _HIP.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    assert _HIP.hipMemset(d_ptr, 0xFF, nbytes) == 0
    assert _HIP.hipDeviceSynchronize() == 0


def _run(path, inp, opts, arith):
    ani = ani_hip.ANI(path, 0)
    ani.set_option("mlp_arith", arith)
    for k, v in opts.items():
        ani.set_option(k, v)
    first = ani.compute(inp, ago=0)
    v = ani.debug_view()
    _poison(v.d_gaev, v.nrows * v.aev_stride * 4)
    out = ani.compute(inp, ago=1)
    assert np.array_equal(out["eatom"], first["eatom"]), "energies changed after dE/dAEV was poisoned"
    assert np.all(np.isfinite(out["force"])), "a poisoned dE/dAEV row was read"
    assert np.abs(out["force"] - first["force"]).max() < 1e-4
    full, rows, v, cm = sr.full_width_rows(ani, inp.nlocal)
    gaev = ani.debug_read(v.d_gaev, (v.nrows, v.aev_stride), np.float32)
    out.update(kernel=ani.last_mlp_kernel(), full=full, rows=rows, nrows=v.nrows, A=v.aev_active_length, cm=cm, gaev_rows=gaev)
    ani.close()
    return out


_REFS = {}


def _reference(path, model, full, species, arith):
    key = (path, hashlib.sha1(full.tobytes()).hexdigest(), arith)
    if key not in _REFS:
        _REFS[key] = sr.mlp_stage(model, full, species, arith=arith)
    return _REFS[key]


def _check_stage(form, arith, box, model_cache):
    path = _model(box, model_cache)
    model = mf.read_model(path)
    inp = _input(box)
    nl = inp.nlocal
    sp = inp.species[:nl]
    got = _run(path, inp, FORMS[form], arith)
    assert got["kernel"].startswith(_expected_kernel(form, arith, model.num_models, nl)), got["kernel"]
    ref = _reference(path, model, got["full"], sp, 1 if arith == 0 else arith)
    A, cm, rows = got["A"], got["cm"], got["rows"]
    g = got["gaev_rows"]
    re = sr.worst_ratio(got["eatom"], ref["eatom"], ref["eatom_bar"])
    rg = sr.worst_ratio(g[rows, :A], ref["gaev"][:, cm], ref["gaev_bar"][:, cm])
    key = (form, arith)
    WORST[key] = max(WORST.get(key, 0.0), re, rg)
    assert re < 1, f"eatom: worst error / bar = {re:.3g} ({got['kernel']})"
    assert rg < 1, f"dE/dAEV: worst error / bar = {rg:.3g} ({got['kernel']})"
    # bucket bookkeeping + padding contract
    kern = got["kernel"]
    block = 32 if kern.startswith("mlp_fused16") else 128
    for s in range(model.num_species):
        r = np.sort(rows[sp == s])
        if r.size == 0:
            continue
        assert np.array_equal(r, np.arange(r[0], r[0] + r.size)), f"rows of species {s} are not contiguous"
        pad = np.arange(r[0] + r.size, r[0] + -(-r.size // block) * block)
        assert np.all(g[pad] == 0), f"padding rows of species {s} after its last atom are not zero ({kern})"


EDGE = "ani2x-m8-all7"


@pytest.mark.parametrize("arith", [1, 2], ids=["arith1-bf16x3", "arith2-f16x2"])
@pytest.mark.parametrize("form", list(FORMS), ids=list(FORMS))
def test_mlp_stage_every_form_on_the_edge_box(form, arith, model_cache):
    _check_stage(form, arith, EDGE, model_cache)


@pytest.mark.parametrize("form", ["m0-chain0", "m0-chain1"])
def test_mlp_stage_fp32_products(form, model_cache):
    """mlp_arith 0: fp32 MFMA products, one rounding each -- inside the bf16x3 bars (rho 2u >= u, the same accumulation)"""
    _check_stage(form, 0, EDGE, model_cache)


@pytest.mark.parametrize("arith", [1, 2], ids=["arith1-bf16x3", "arith2-f16x2"])
@pytest.mark.parametrize("form", ["default", "m2-g0", "m2-g1-r64-h2", "m0-chain1"])
@pytest.mark.parametrize("box", [b for b in BOXES if b != EDGE])
def test_mlp_stage_edge_boxes(box, form, arith, model_cache):
    _check_stage(form, arith, box, model_cache)


@pytest.mark.parametrize("arith", [1, 2], ids=["arith1-bf16x3", "arith2-f16x2"])
def test_mlp_stage_large_water_default_schedule(arith, model_cache):
    """50 001 water atoms, one member, the default options: the schedule the library picks for a size where it may cut items
    in two (whether it does is decided by timing both schedules; mlp_fused_halves 2 above forces the halves)"""
    _check_stage("default", arith, "water-50001-m1", model_cache)


# ---- repeatability -------------------------------------------------------------------------------------------------------

def _gaev_eatom(ani, inp, ago):
    out = ani.compute(inp, ago=ago)
    v = ani.debug_view()
    return ani.debug_read(v.d_gaev, (v.nrows, v.aev_stride), np.float32), out["eatom"].copy(), v, ani.debug_read(v.d_row_of_centre, (inp.nlocal,), np.int32)


@pytest.mark.parametrize("members", [1, 8], ids=["m1-water1500", "m8-water600"])
@pytest.mark.parametrize("arith", [1, 2], ids=["arith1-bf16x3", "arith2-f16x2"])
@pytest.mark.parametrize("form", FUSED, ids=FUSED)
def test_fused_forms_repeat_bit_for_bit(form, arith, members, model_cache):
    """20 evaluations at ago = 1 give the same bits: real rows of dE/dAEV and every atom's energy (round 4 found a data race
    in the sixteen-row kernel's LDS-DMA form that returned wrong rows in about half of the evaluations, water-1500).  Eight
    members: the (tile, member) work items, each member's own dE/dAEV copy and the kernel that sums them (mlp_fused 2), or
    the members one after the other in a workgroup (mlp_fused 3)."""
    path = model_cache("ani2x", members, 2024)
    inp = hx.decompose(hx.water_box(1500 if members == 1 else 600, seed=5))
    ani = ani_hip.ANI(path, 0)
    ani.set_option("mlp_arith", arith)
    for k, v in FORMS[form].items():
        ani.set_option(k, v)
    g0, e0, v, rows = _gaev_eatom(ani, inp, 0)
    assert ani.last_mlp_kernel().startswith(_expected_kernel(form, arith, members, inp.nlocal)), ani.last_mlp_kernel()
    bad = 0
    for _ in range(20):
        g, e, _, _ = _gaev_eatom(ani, inp, 1)
        bad += int(not (np.array_equal(g[rows], g0[rows]) and np.array_equal(e, e0)))
    ani.close()
    assert bad == 0, f"{bad} of 20 evaluations differ from the first"


def _rows_and_eatom(path, inp, opts, arith):
    o = _run(path, inp, opts, arith)
    return o["gaev_rows"][o["rows"]], o["eatom"], o["kernel"]


@pytest.mark.parametrize("arith", [1, 2], ids=["arith1-bf16x3", "arith2-f16x2"])
def test_sixteen_row_kernel_128_and_64_row_forms_agree_bit_for_bit(arith, model_cache):
    """mlp_fused16<P, 8> and <P, 4>: the same per-wave arithmetic in the same order on 16-row strips (tools/mlpg_debug.py)"""
    path = model_cache("ani2x", 1, 2024)
    inp = hx.decompose(hx.water_box(1500, seed=5))
    a = _rows_and_eatom(path, inp, dict(mlp_fused=2, mlp_fused_rows=128, mlp_fused_halves=0, **G), arith)
    b = _rows_and_eatom(path, inp, dict(mlp_fused=2, mlp_fused_rows=64, mlp_fused_halves=0, **G), arith)
    assert a[2].endswith(", 8>") and b[2].endswith(", 4>")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("gen", [1, 0], ids=["gen1", "gen0"])
@pytest.mark.parametrize("arith", [1, 2], ids=["arith1-bf16x3", "arith2-f16x2"])
def test_mlp_fused_1_and_2_agree_bit_for_bit_with_eight_members(arith, gen, model_cache):
    """eight members: mlp_fused 1 (default) runs the same (tile, member) work items as mlp_fused 2"""
    path = model_cache("ani2x", 8, 7)
    inp = hx.decompose(hx.water_box(600, seed=2))
    a = _rows_and_eatom(path, inp, dict(mlp_fused=1, mlp_fused_gen=gen), arith)
    b = _rows_and_eatom(path, inp, dict(mlp_fused=2, mlp_fused_gen=gen), arith)
    assert a[2] == b[2]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("arith", [1, 2], ids=["arith1-bf16x3", "arith2-f16x2"])
def test_one_handle_across_list_epochs_agrees_bit_for_bit_with_fresh_handles(arith, model_cache):
    """One handle through five list epochs (ago = 0) that change the tile counts, the species present (the weight streams are
    re-made for the pruned AEV layout) and the schedule's options: what it keeps between epochs -- the static schedule and its
    key, the streams -- must give the bits of a fresh handle with the same options on the same box, real rows of dE/dAEV and
    every atom's energy.  Per-species counts on different tile edges in both boxes; mlp_fused_halves 0 or 2 only, so no timed
    decision enters."""
    path = model_cache("ani2x", 2, 41)
    X = hx.decompose(_system([129, 15, 1, 64, 33, 127, 17]))     # 386 atoms
    Y = hx.decompose(_system([257, 31, 0, 128, 65, 16, 63]))     # 560 atoms, one species absent
    P = 3 if arith == 1 else 2
    opts = dict(mlp_fused=2, mlp_fused_rows=128, mlp_fused_halves=0, **G)
    steps = [(X, {}, 8), (Y, {}, 8), (X, {}, 8), (X, dict(mlp_fused_halves=2), 8), (Y, dict(mlp_fused_rows=64), 4)]
    ani = ani_hip.ANI(path, 0)
    ani.set_option("mlp_arith", arith)
    for k, v in opts.items():
        ani.set_option(k, v)
    for i, (inp, change, waves) in enumerate(steps):
        opts.update(change)
        for k, v in change.items():
            ani.set_option(k, v)
        g, e, _, rows = _gaev_eatom(ani, inp, 0)
        assert ani.last_mlp_kernel() == "mlp_fused16<%d, %d>" % (P, waves), (i + 1, ani.last_mlp_kernel())
        fresh = ani_hip.ANI(path, 0)
        fresh.set_option("mlp_arith", arith)
        for k, v in opts.items():
            fresh.set_option(k, v)
        g0, e0, _, rows0 = _gaev_eatom(fresh, inp, 0)
        assert fresh.last_mlp_kernel() == ani.last_mlp_kernel()
        fresh.close()
        assert np.array_equal(rows, rows0)
        assert np.array_equal(g[rows], g0[rows0]), f"step {i + 1}: dE/dAEV rows differ from a fresh handle's"
        assert np.array_equal(e, e0), f"step {i + 1}: energies differ from a fresh handle's"
    ani.close()
