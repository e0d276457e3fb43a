"""The LAMMPS-side adapter (lammps-ani_amd/csrc/pair_ani.cpp + ani_plugin.cpp) driven through mock LAMMPS objects
(tests/mock_lammps).  Mirrors what LAMMPS' test_pair_style does with the reference's yaml files
(tests/lammps-unittest/*/): init forces/energy/stress of the 30-atom water box, restart round trip, newton checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import golden_input, golden_model_path, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "mock_lammps")


@pytest.fixture(scope="module")
def mock():
    from lammps_ani_amd import ani_hip
    ani_hip.build()
    subprocess.check_call(["make", "-C", MOCK, "-s"])
    lib = C.CDLL(os.path.join(MOCK, "libpair_ani_mock.so"))
    lib.mock_create.restype = C.c_void_p
    lib.mock_create.argtypes = [C.c_char_p, C.c_int]
    lib.mock_error.restype = C.c_char_p
    lib.mock_error.argtypes = [C.c_void_p]
    lib.mock_plugin_name.restype = C.c_char_p
    lib.mock_pair_style.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_int]
    lib.mock_last_request.argtypes = [C.c_void_p]
    lib.mock_init_one.argtypes = [C.c_void_p]
    lib.mock_init_one.restype = C.c_double
    lib.mock_compute.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.mock_restart_roundtrip.argtypes = [C.c_void_p, C.c_char_p]
    lib.mock_destroy.argtypes = [C.c_void_p]
    lib.mock_set_ilist.argtypes = [C.c_void_p, C.c_void_p]
    return lib


def _style(lib, h, args, ntypes=7):
    arr = (C.c_char_p * len(args))(*[a.encode() for a in args])
    rc = lib.mock_pair_style(h, len(args), arr, ntypes)
    return rc, lib.mock_error(h).decode()


def test_adapter_rejects_bad_input_without_gpu(mock):
    """Host-side checks that need no device (reference src/pair_ani.cpp:44-46, 285-341)."""
    h = mock.mock_create(b"metal", 0)
    rc, err = _style(mock, h, ["5.1", "/nonexistent.anim", "hip"])
    assert rc == 1 and "real units" in err
    h = mock.mock_create(b"real", 0)
    rc, err = _style(mock, h, ["5.1", "/nonexistent.anim", "cpu"])
    assert rc == 1 and "cpu" in err
    rc, err = _style(mock, h, ["5.1", "/nonexistent.anim", "hip", "-1", "fastaev"])
    assert rc == 1 and "cuaev or pyaev" in err
    rc, err = _style(mock, h, ["5.1", "/nonexistent.anim", "hip", "-1", "cuaev", "quarter"])
    assert rc == 1 and "full or half" in err
    rc, err = _style(mock, h, ["5.1"])
    assert rc == 1 and "Illegal pair_style" in err


def _run(mock, h, inp, ago, eflag=3, vflag=1):
    nt = inp.ntotal
    f = np.zeros((nt, 3))
    e = np.zeros(1)
    v = np.zeros(6)
    ea = np.zeros(inp.nlocal)
    x = np.ascontiguousarray(inp.x)
    ty = np.ascontiguousarray(inp.types, dtype=np.int32)
    nn = np.ascontiguousarray(inp.numneigh, dtype=np.int32)
    jl = np.ascontiguousarray(inp.jlist, dtype=np.int32)
    ow = np.ascontiguousarray(inp.owner_lidx, dtype=np.int32)
    rc = mock.mock_compute(h, inp.nlocal, inp.nghost, x.ctypes.data, ty.ctypes.data, nn.ctypes.data, jl.ctypes.data,
                           ow.ctypes.data, ago, eflag, vflag, f.ctypes.data, e.ctypes.data, v.ctypes.data, ea.ctypes.data)
    assert rc == 0, mock.mock_error(h).decode()
    return f, float(e[0]), v, ea


@pytest.mark.gpu
@pytest.mark.parametrize("nbr", ["full", "half"])
@pytest.mark.parametrize("aev", ["cuaev", "pyaev"])
def test_adapter_matches_golden_water30(mock, model_cache, nbr, aev):
    """`pair_style ani 5.1 <model> hip -1 <aev> <nbr> single` on tests/golden/water-0.8nm.data, PBC 8 A: forces after the
    adapter's own reverse communication, eng_vdwl, virial (xx yy zz xy xz yz), eatom — against the fp64 fixtures."""
    g = load_golden("water30_pbc_ani2x_m8")
    inp = golden_input(g, half=(nbr == "half"))
    p = golden_model_path(g, model_cache)
    h = mock.mock_create(b"real", 0)
    rc, err = _style(mock, h, ["5.1", p, "hip", "-1", aev, nbr, "single"])
    assert rc == 0, err
    assert mock.mock_plugin_name() == b"ani"
    assert mock.mock_last_request(h) == (1 if nbr == "full" else 0)  # REQ_FULL vs default half request
    assert mock.mock_init_one(h) == 5.1
    mode = "strict" if aev == "cuaev" else "compat"
    ref_f = g[f"{mode}_force"]
    folded = ref_f[: inp.nlocal].copy()
    np.add.at(folded, inp.owner_lidx, ref_f[inp.nlocal:])
    vref = g[f"{mode}_virial"]
    for ago in (0, 1):
        f, e, v, ea = _run(mock, h, inp, ago)
        assert abs(e - float(g[f"{mode}_energy"])) < 2e-3
        np.testing.assert_allclose(f[: inp.nlocal], folded, rtol=0, atol=2.3e-3)
        np.testing.assert_allclose(v, [vref[0, 0], vref[1, 1], vref[2, 2], vref[0, 1], vref[0, 2], vref[1, 2]], rtol=0, atol=2e-2)
        np.testing.assert_allclose(ea, g[f"{mode}_eatom"], rtol=0, atol=2e-3)
    # restart round trip re-creates the model from the stored path and settings (src/pair_ani.cpp:408-455)
    assert mock.mock_restart_roundtrip(h, b"/tmp/_pair_ani_restart.bin") == 0, mock.mock_error(h).decode()
    f2, e2, _, _ = _run(mock, h, inp, 0)
    np.testing.assert_allclose(f2, f, rtol=0, atol=1e-3)  # float atomics: not bitwise
    assert abs(e2 - e) < 1e-6
    mock.mock_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["reversed", "random"])
def test_adapter_with_an_ilist_that_is_not_the_identity(mock, model_cache, order):
    """LAMMPS hands the centres over in list->ilist order, with numneigh / firstneigh indexed by ATOM.  The adapter gathers
    numneigh[ilist[ii]] and firstneigh[ilist[ii]] into the library's ilist-ordered arrays and scatters the per-centre energies
    back through ilist (the reference's "numneigh indexing wart", SURVEY.md section 7, only agrees with LAMMPS for the identity).
    Full list, per-atom energies: forces, eng_vdwl, virial and eatom BY ATOM against the fp64 fixture, over a rebuild in that
    order, a cached step, and a rebuild back in the identity order."""
    g = load_golden("water30_pbc_ani2x_m8")
    inp = golden_input(g, half=False)
    p = golden_model_path(g, model_cache)
    nl = inp.nlocal
    ilist = np.arange(nl)[::-1] if order == "reversed" else np.random.default_rng(30).permutation(nl)
    ilist = np.ascontiguousarray(ilist, dtype=np.int32)
    assert np.array_equal(np.sort(ilist), np.arange(nl)) and int((ilist == np.arange(nl)).sum()) <= 2
    eref = g["strict_eatom"]
    assert np.abs(eref - eref[ilist]).max() > 1000 * 2e-3   # eatom left in ilist order would miss by the H / O self energies
    h = mock.mock_create(b"real", 0)
    rc, err = _style(mock, h, ["5.1", p, "hip", "-1", "cuaev", "full", "single"])
    assert rc == 0, err
    ref_f = g["strict_force"]
    folded = ref_f[:nl].copy()
    np.add.at(folded, inp.owner_lidx, ref_f[nl:])
    vref = g["strict_virial"]
    for ago, permuted in ((0, True), (1, True), (0, False)):
        if ago == 0 and permuted:
            mock.mock_set_ilist(h, ilist.ctypes.data)
        f, e, v, ea = _run(mock, h, inp, ago)
        assert abs(e - float(g["strict_energy"])) < 2e-3
        np.testing.assert_allclose(f[:nl], folded, rtol=0, atol=2.3e-3)
        np.testing.assert_allclose(v, [vref[0, 0], vref[1, 1], vref[2, 2], vref[0, 1], vref[0, 2], vref[1, 2]], rtol=0, atol=2e-2)
        np.testing.assert_allclose(ea, eref, rtol=0, atol=2e-3)
    mock.mock_destroy(h)


@pytest.mark.gpu
def test_adapter_requires_newton_pair_off(mock, model_cache):
    p = model_cache("tiny", 2, 5)
    h = mock.mock_create(b"real", 1)
    rc, err = _style(mock, h, ["5.1", p, "hip", "-1", "cuaev", "full"], ntypes=3)
    assert rc == 1 and "newton pair off" in err


@pytest.mark.gpu
def test_adapter_double_precision(mock, model_cache):
    """`... half double`, the configuration of the reference's fp64 yaml files."""
    g = load_golden("water30_pbc_ani2x_m8")
    inp = golden_input(g, half=True)
    p = golden_model_path(g, model_cache)
    h = mock.mock_create(b"real", 0)
    rc, err = _style(mock, h, ["5.1", p, "hip", "-1", "pyaev", "half", "double"])
    assert rc == 0, err
    f, e, v, ea = _run(mock, h, inp, 0)
    ref_f = g["compat_force"]
    folded = ref_f[: inp.nlocal].copy()
    np.add.at(folded, inp.owner_lidx, ref_f[inp.nlocal:])
    assert abs(e - float(g["compat_energy"])) < 9e-9 * abs(float(g["compat_energy"]))
    np.testing.assert_allclose(f[: inp.nlocal], folded, rtol=0, atol=1e-8)
    mock.mock_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("aev", ["cuaev", "pyaev"])
def test_adapter_devlist_matches_hostlist(mock, model_cache, aev):
    """`... full single devlist`: LAMMPS is asked for an occasional list only (never built) and the list comes from
    ani_build_list on the device; forces / energy / virial / eatom equal the host-list run and the fp64 fixtures."""
    g = load_golden("water30_pbc_ani2x_m8")
    inp = golden_input(g, half=False)
    p = golden_model_path(g, model_cache)
    out = {}
    for src in ("hostlist", "devlist"):
        h = mock.mock_create(b"real", 0)
        rc, err = _style(mock, h, ["5.1", p, "hip", "-1", aev, "full", "single", src])
        assert rc == 0, err
        assert mock.mock_last_request(h) == (1 if src == "hostlist" else (1 | 16))  # REQ_FULL [| REQ_OCCASIONAL]
        for ago in (0, 1, 0):
            out[src] = _run(mock, h, inp, ago)
        mock.mock_destroy(h)
    (fh, eh, vh, eah), (fd, ed, vd, ead) = out["hostlist"], out["devlist"]
    np.testing.assert_allclose(fd, fh, rtol=0, atol=1e-3)   # same pairs, another summation order
    assert abs(ed - eh) < 1e-3
    np.testing.assert_allclose(vd, vh, rtol=0, atol=1e-2)
    np.testing.assert_allclose(ead, eah, rtol=0, atol=1e-3)
    mode = "strict" if aev == "cuaev" else "compat"
    ref_f = g[f"{mode}_force"]
    folded = ref_f[: inp.nlocal].copy()
    np.add.at(folded, inp.owner_lidx, ref_f[inp.nlocal:])
    np.testing.assert_allclose(fd[: inp.nlocal], folded, rtol=0, atol=2.3e-3)
    h = mock.mock_create(b"real", 0)
    rc, err = _style(mock, h, ["5.1", p, "hip", "-1", aev, "half", "single", "devlist"])
    assert rc == 1 and "full" in err
    rc, err = _style(mock, h, ["5.1", p, "hip", "-1", aev, "full", "single", "gpulist"])
    assert rc == 1 and "hostlist or devlist" in err


@pytest.mark.gpu
@pytest.mark.parametrize("nbr", ["full", "half"])
def test_adapter_rcclcomm_matches_mpicomm(mock, model_cache, nbr, monkeypatch):
    """`... single hostlist rcclcomm`: the ghost-force reverse communication runs on the device through include/ani_comm.h
    (owners found with comm->forward_comm(this), maps handed to the library per re-neighbouring, forces summed before the
    D2H copy) instead of comm->reverse_comm(this) on the host (src/pair_ani.cpp:197-201,461-484).  One rank: the ghosts are
    the box's periodic images, their owner is this rank; forces of the owned atoms must equal the host path's and the
    fixtures, and the ghost rows must come back untouched (nothing left to reverse-communicate)."""
    g = load_golden("water30_pbc_ani2x_m8")
    inp = golden_input(g, half=(nbr == "half"))
    p = golden_model_path(g, model_cache)
    out = {}
    # "mpicomm" on ONE rank sums the images on the device too (a communicator without RCCL); LAMMPS_ANI_NO_SELF_FOLD keeps
    # comm->reverse_comm(this) on the host, the reference's path and the yardstick here
    for mode in ("mpicomm host", "mpicomm", "rcclcomm"):
        if mode == "mpicomm host":
            monkeypatch.setenv("LAMMPS_ANI_NO_SELF_FOLD", "1")
        else:
            monkeypatch.delenv("LAMMPS_ANI_NO_SELF_FOLD", raising=False)
        h = mock.mock_create(b"real", 0)
        rc, err = _style(mock, h, ["5.1", p, "hip", "-1", "cuaev", nbr, "single", "hostlist", mode.split()[0]])
        assert rc == 0, err
        for ago in (0, 1, 0):
            out[mode] = _run(mock, h, inp, ago)
        mock.mock_destroy(h)
    (fm, em, vm, _), (fr, er, vr, _) = out["mpicomm host"], out["rcclcomm"]
    fs, es, vs, _ = out["mpicomm"]
    np.testing.assert_allclose(fs[: inp.nlocal], fm[: inp.nlocal], rtol=0, atol=1e-3)
    assert np.all(fs[inp.nlocal:] == 0.0) and abs(es - em) < 1e-6
    np.testing.assert_allclose(vs, vm, rtol=0, atol=1e-2)
    np.testing.assert_allclose(fr[: inp.nlocal], fm[: inp.nlocal], rtol=0, atol=1e-3)
    assert np.all(fr[inp.nlocal:] == 0.0)
    assert abs(er - em) < 1e-6
    np.testing.assert_allclose(vr, vm, rtol=0, atol=1e-2)
    ref_f = g["strict_force"]
    folded = ref_f[: inp.nlocal].copy()
    np.add.at(folded, inp.owner_lidx, ref_f[inp.nlocal:])
    np.testing.assert_allclose(fr[: inp.nlocal], folded, rtol=0, atol=2.3e-3)
    h = mock.mock_create(b"real", 0)
    rc, err = _style(mock, h, ["5.1", p, "hip", "-1", "cuaev", nbr, "single", "hostlist", "ucxcomm"])
    assert rc == 1 and "mpicomm or rcclcomm" in err


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["hostlist", "devlist"])
def test_adapter_device_fold_and_direct_accumulation_at_a_size_that_takes_the_polled_copy(mock, model_cache, source, monkeypatch):
    """6 000 water atoms (above the 4 096 rows from which the library brings the forces over by its copy-out kernel and adds them
    into atom->f chunk by chunk): the one-rank default (device fold through a communicator without RCCL, direct accumulation)
    against the host path (LAMMPS_ANI_NO_SELF_FOLD: full download, comm->reverse_comm, f += out_force), over a rebuild, two cached
    steps and another rebuild.  f carries a non-zero start value in neither (the mock clears it, like LAMMPS' force_clear)."""
    from lammps_ani_amd import harness as hx
    inp = hx.decompose(hx.spatial_sort(hx.water_box(6000, seed=5)))
    p = model_cache("ani2x", 2, 2024)
    out = {}
    for mode in ("host", "fold"):
        if mode == "host":
            monkeypatch.setenv("LAMMPS_ANI_NO_SELF_FOLD", "1")
        else:
            monkeypatch.delenv("LAMMPS_ANI_NO_SELF_FOLD", raising=False)
        h = mock.mock_create(b"real", 0)
        rc, err = _style(mock, h, ["5.1", p, "hip", "-1", "cuaev", "full", "single", source])
        assert rc == 0, err
        out[mode] = [_run(mock, h, inp, ago) for ago in (0, 1, 2, 0)]
        mock.mock_destroy(h)
    for (fh, eh, vh, eah), (ff, ef, vf, eaf) in zip(out["host"], out["fold"]):
        np.testing.assert_allclose(ff[: inp.nlocal], fh[: inp.nlocal], rtol=0, atol=2e-4)
        assert np.all(ff[inp.nlocal:] == 0.0)              # nothing left in the ghost rows: the images went home on the device
        assert abs(ef - eh) < 1e-6 * max(1.0, abs(eh))
        np.testing.assert_allclose(vf, vh, rtol=1e-6, atol=1e-2)
        np.testing.assert_allclose(eaf, eah, rtol=0, atol=1e-6)
