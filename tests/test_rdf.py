"""GPU: the RDF accumulators (ani_rdf_* of include/ani_hip.h, kernel in ani_kernels_rdf.hip) against the brute-force reference
tests/rdf_reference.py.  The results are integers: every comparison is an equality.

The cases are those of rdf_reference.case(); tests/test_rdf_reference_cpu.py pins, on the CPU, that none of them has a pair within
1e-9 A of a bin edge (so the fp64 arithmetic of the two sides cannot disagree about a bin) and writes their totals down.  Every
read goes through ctypes into buffers with sentinels behind each array."""
import ctypes as C

import numpy as np
import pytest

import rdf_reference as rr
from lammps_ani_amd import harness as hx

pytestmark = pytest.mark.gpu

SENT = np.uint64(0xA5A5A5A5A5A5A5A5)
GAP = 1e-9
ANI_ERR_ARG = 1


@pytest.fixture(scope="module")
def hip():
    from lammps_ani_amd import ani_hip
    return ani_hip


def make(hip, model_cache, **kw):
    return hip.ANI(model_cache("ani2x", 1, 11), 0, **kw)


def raw_read(ani, npair, nbins, reset=0, pad=5):
    """ani_rdf_read through ctypes with sentinels behind every output: (rc, counts, centres, frames)"""
    counts = np.full(npair * nbins + pad, SENT, dtype=np.uint64)
    centres = np.full(npair + pad, SENT, dtype=np.uint64)
    frames = np.full(1 + pad, SENT, dtype=np.uint64)
    rc = ani._lib.ani_rdf_read(ani._h, counts.ctypes.data, centres.ctypes.data, frames.ctypes.data, int(reset))
    assert (counts[npair * nbins:] == SENT).all() and (centres[npair:] == SENT).all() and (frames[1:] == SENT).all()
    return rc, counts[: npair * nbins].reshape(npair, nbins), centres[:npair], int(frames[0])


def configure(ani, c):
    assert c.gap > GAP
    ani.rdf_configure(c.nbins, c.rmax, c.pairs)


def check(ani, c, nframes=1, reset=0):
    rc, counts, centres, frames = raw_read(ani, len(c.pairs), c.nbins, reset)
    print("totals", counts.sum(1).tolist(), "reference x", nframes, c.totals, "centres", centres.tolist(), "frames", frames)
    assert rc == 0, ani._lib.ani_last_error(ani._h)
    assert frames == nframes
    assert np.array_equal(centres, c.centres * np.uint64(nframes))
    assert np.array_equal(counts, c.counts * np.uint64(nframes))
    return counts, centres, frames


def _list_layout(ani, nlocal):
    pn, po, pj = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert ani._lib.ani_debug_list(ani._h, C.byref(pn), C.byref(po), C.byref(pj)) == 0
    nn = ani.debug_read(pn, (nlocal,), np.int32)
    off = ani.debug_read(po, (nlocal + 1,), np.int32)
    return "dense" if np.array_equal(np.diff(off), nn) else "rows"


def test_random_box_callers_list(model_cache, hip):
    """case 1a: one rank, periodic, all 16 ordered pairs, the caller's list installed by a step (dense segments); 600 centres x 16
    lanes leave the last workgroup partly empty.  The host entry, then the device entry and the python read."""
    import torch
    c = rr.case("random")
    inp = c.obj
    assert inp.nlocal * 16 % 256 != 0
    ani = make(hip, model_cache)
    ani.compute(inp, ago=0)
    configure(ani, c)
    ani.rdf_accumulate(inp)
    check(ani, c, reset=1)
    d_x = torch.as_tensor(inp.x, dtype=torch.float64, device=torch.device("cuda:0")).contiguous()
    ani.rdf_accumulate_device(inp.ntotal, inp.nlocal, d_x.data_ptr())
    counts, centres, frames = ani.rdf_read()
    assert frames == 1 and counts.dtype == np.uint64 and counts.shape == (16, 64) and centres.shape == (16,)
    assert np.array_equal(counts, c.counts) and np.array_equal(centres, c.centres)
    # a wave per centre, and the global-atomics path at this size: measurement options, same words
    for name, value in (("rdf_lanes", 64), ("rdf_lds", 0)):
        ani.set_option(name, value)
        ani.rdf_read(reset=True)
        ani.rdf_accumulate(inp)
        check(ani, c)
    ani.close()


def test_random_box_built_lists(model_cache, hip):
    """case 1b: the library's own list, in both of its layouts (dense segments, capacity rows)"""
    c = rr.case("random")
    inp = c.obj
    ani = make(hip, model_cache)
    configure(ani, c)
    layouts = []
    for k in range(3):
        assert ani.build_list(inp.species, inp.x, inp.nlocal, 7.1) == inp.npairs
        layouts.append(_list_layout(ani, inp.nlocal))
        ani.rdf_accumulate(inp)
        check(ani, c, nframes=k + 1)      # the accumulators outlive a list epoch
    print("layouts", layouts)
    assert "rows" in layouts and "dense" in layouts
    ani.close()


@pytest.mark.parametrize("name", ["random_4096", "random_subset"])
def test_global_path_and_subset(name, model_cache, hip):
    """case 2: 16 pairs x 4096 bins count straight into global memory; 3 pairs with one centre species twice, rmax 2.0"""
    c = rr.case(name)
    assert (len(c.pairs) * c.nbins > 8192) == (name == "random_4096")
    ani = make(hip, model_cache)
    ani.compute(c.obj, ago=0)
    configure(ani, c)
    ani.rdf_accumulate(c.obj)
    check(ani, c)
    ani.close()


def test_frames_reset_reconfigure(model_cache, hip):
    """case 3"""
    c, sub = rr.case("random"), rr.case("random_subset")
    ani = make(hip, model_cache)
    ani.compute(c.obj, ago=0)
    configure(ani, c)
    for _ in range(3):
        ani.rdf_accumulate(c.obj)
    check(ani, c, nframes=3, reset=1)
    rc, counts, centres, frames = raw_read(ani, 16, 64)
    assert rc == 0 and frames == 0 and not counts.any() and not centres.any()
    ani.rdf_accumulate(c.obj)
    check(ani, c)                         # the configuration was kept
    configure(ani, sub)                   # reconfiguring discards
    rc, counts, centres, frames = raw_read(ani, 3, 64)
    assert rc == 0 and frames == 0 and not counts.any() and not centres.any()
    ani.rdf_accumulate(sub.obj)
    check(ani, sub)
    # cleared: nothing to read, nothing to accumulate into
    ani.rdf_configure(1, 1.0, [])
    rc = ani._lib.ani_rdf_accumulate(ani._h, c.obj.ntotal, c.obj.nlocal, np.ascontiguousarray(c.obj.x).ctypes.data)
    assert rc == ANI_ERR_ARG and b"nothing is configured" in ani._lib.ani_last_error(ani._h)
    with pytest.raises(hip.AniError, match="nothing is configured"):
        ani.rdf_read()
    ani.close()


def test_second_run_is_bitwise_the_same(model_cache, hip):
    """case 4"""
    c = rr.case("random")
    words = []
    for _ in range(2):
        ani = make(hip, model_cache)
        ani.compute(c.obj, ago=0)
        configure(ani, c)
        ani.rdf_accumulate(c.obj)
        ani.rdf_accumulate(c.obj)
        rc, counts, centres, frames = raw_read(ani, 16, 64)
        assert rc == 0
        words.append(counts.tobytes() + centres.tobytes() + frames.to_bytes(8, "little"))
        ani.close()
    assert words[0] == words[1]


def test_outputs_may_be_left_out(model_cache, hip):
    """case 5: any output pointer may be NULL; nothing is written past npair * nbins, npair or 1 (raw_read's sentinels, here with
    each array alone)"""
    c = rr.case("random_subset")
    ani = make(hip, model_cache)
    ani.compute(c.obj, ago=0)
    configure(ani, c)
    ani.rdf_accumulate(c.obj)
    lib, h = ani._lib, ani._h
    n = 3 * 64
    buf = np.full(n + 7, SENT, dtype=np.uint64)
    assert lib.ani_rdf_read(h, buf.ctypes.data, None, None, 0) == 0
    assert np.array_equal(buf[:n].reshape(3, 64), c.counts) and (buf[n:] == SENT).all()
    buf = np.full(3 + 7, SENT, dtype=np.uint64)
    assert lib.ani_rdf_read(h, None, buf.ctypes.data, None, 0) == 0
    assert np.array_equal(buf[:3], c.centres) and (buf[3:] == SENT).all()
    buf = np.full(1 + 7, SENT, dtype=np.uint64)
    assert lib.ani_rdf_read(h, None, None, buf.ctypes.data, 0) == 0
    assert buf[0] == 1 and (buf[1:] == SENT).all()
    assert lib.ani_rdf_read(h, None, None, None, 1) == 0       # only the reset
    rc, counts, centres, frames = raw_read(ani, 3, 64)
    assert rc == 0 and frames == 0 and not counts.any() and not centres.any()
    ani.close()


def test_own_images_and_empty_rank(model_cache, hip):
    """case 6: one atom alone in a periodic 4 A box, ghosts by hx.decompose -- its own images are its only neighbours and they are
    counted; and a rank that owns nothing: a frame, no counts"""
    import torch
    c = rr.case("one_atom")
    inp = c.obj
    assert inp.nlocal == 1 and inp.nghost == 124 and c.totals == [6]
    ani = make(hip, model_cache)
    ani.compute(inp, ago=0)
    configure(ani, c)
    ani.rdf_accumulate(inp)
    check(ani, c)
    # nlocal == 0: every atom a ghost
    dev = torch.device("cuda:0")
    x = torch.as_tensor(inp.x, dtype=torch.float64, device=dev).contiguous()
    sp = torch.as_tensor(inp.species.astype(np.int32), device=dev)
    n = ani.build_list_device(inp.ntotal, 0, sp.data_ptr(), x.data_ptr(), 7.1, inp.x.min(0) - 0.25, inp.x.max(0) + 0.25)
    assert n == 0
    ani.rdf_accumulate_device(inp.ntotal, 0, x.data_ptr())
    rc, counts, centres, frames = raw_read(ani, 1, 64)
    assert rc == 0 and frames == 2
    assert np.array_equal(counts, c.counts) and np.array_equal(centres, c.centres)   # what the first frame left
    ani.close()


def test_two_ranks_add_up(model_cache, hip):
    """case 7: rank 0 and rank 1 of a (2,1,1) grid one after the other on one card; each equals its reference, their sum the box"""
    whole = rr.case("random_whole")
    total = np.zeros_like(whole.counts)
    total_c = np.zeros_like(whole.centres)
    for name in ("rank0", "rank1"):
        c = rr.case(name)
        ani = make(hip, model_cache)
        ani.compute(c.obj, ago=0)
        configure(ani, c)
        ani.rdf_accumulate(c.obj)
        counts, centres, _ = check(ani, c)
        total += counts
        total_c += centres
        ani.close()
    assert np.array_equal(total, whole.counts) and np.array_equal(total_c, whole.centres)


def test_non_identity_ilist(model_cache, hip):
    """case 8: the centres in a random order with every segment shuffled (tests/list_forms.py): the same counts"""
    import list_forms as lf
    c = rr.case("random")
    inp, perm = lf.apply_form(c.obj, "random+shuffled")
    assert lf.longest_fixed_run(perm) < 4 and not np.array_equal(inp.jlist, c.obj.jlist)
    ani = make(hip, model_cache)
    ani.compute(inp, ago=0)
    configure(ani, c)
    ani.rdf_accumulate(inp)
    check(ani, c)
    ani.close()


def test_refusals(model_cache, hip):
    """case 9: each refusal is ANI_ERR_ARG with a message that names the reason, and the refused call accumulates nothing"""
    c = rr.case("random")
    inp = c.obj
    ani = make(hip, model_cache)
    lib, h = ani._lib, ani._h
    x = np.ascontiguousarray(inp.x)

    def conf(nbins, rmax, pairs):
        p = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        return lib.ani_rdf_configure(h, nbins, C.c_double(rmax), p.ctypes.data, len(p)), lib.ani_last_error(h).decode()

    def acc(a=ani, nt=inp.ntotal, nl=inp.nlocal, xp=x.ctypes.data):
        return a._lib.ani_rdf_accumulate(a._h, nt, nl, xp), a._lib.ani_last_error(a._h).decode()

    rcr = ani.cutoffs()[0]
    assert rcr == pytest.approx(5.1)
    # accumulate before configure
    rc, msg = acc()
    assert rc == ANI_ERR_ARG and "nothing is configured" in msg
    # a good configuration first: every refusal below has to leave it, and its zeros, alone
    assert conf(64, 5.1, rr.ALL16)[0] == 0
    # accumulate with no list
    rc, msg = acc()
    assert rc == ANI_ERR_ARG and "no neighbour list" in msg
    ani.compute(inp, ago=0)
    rc, msg = conf(64, np.nextafter(rcr, 10.0), [(0, 0)])
    assert rc == ANI_ERR_ARG and "rmax" in msg and "cutoff" in msg
    rc, msg = conf(64, 5.2, [(0, 0)])
    assert rc == ANI_ERR_ARG and "rmax" in msg and "5.2" in msg
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        rc, msg = conf(64, bad, [(0, 0)])
        assert rc == ANI_ERR_ARG and "rmax" in msg and "positive finite" in msg
    rc, msg = conf(0, 5.1, [(0, 0)])
    assert rc == ANI_ERR_ARG and "nbins = 0" in msg
    rc, msg = conf(4097, 5.1, [(0, 0)])
    assert rc == ANI_ERR_ARG and "nbins = 4097" in msg and "4096" in msg
    rc, msg = conf(64, 5.1, [(0, 0), (1, 7)])
    assert rc == ANI_ERR_ARG and "species 7" in msg and "pair 1" in msg
    rc, msg = conf(64, 5.1, [(-1, 0)])
    assert rc == ANI_ERR_ARG and "species -1" in msg
    rc, msg = conf(64, 5.1, [(0, 3), (3, 0), (0, 3)])
    assert rc == ANI_ERR_ARG and "twice" in msg and "(H, O)" in msg
    with pytest.raises(hip.AniError, match="no species"):
        ani.rdf_configure(64, 5.1, [("O", "Xe")])
    # ntotal / nlocal mismatch, null positions
    rc, msg = acc(nt=inp.ntotal - 1)
    assert rc == ANI_ERR_ARG and "differ" in msg
    rc, msg = acc(nl=inp.nlocal - 1)
    assert rc == ANI_ERR_ARG and "differ" in msg
    rc, msg = acc(xp=None)
    assert rc == ANI_ERR_ARG and "null positions" in msg
    assert lib.ani_rdf_accumulate_device(h, inp.ntotal, inp.nlocal, None, None) == ANI_ERR_ARG
    # nothing was accumulated by any refused call, and the good configuration stands
    rc, counts, centres, frames = raw_read(ani, 16, 64)
    assert rc == 0 and frames == 0 and not counts.any() and not centres.any()
    assert acc()[0] == 0
    check(ani, c)
    # (a, b) and (b, a) are different pairs; symbols resolve through the model
    ani.rdf_configure(64, 5.1, [("O", "H"), ("H", "O")])
    ani.rdf_accumulate(inp)
    counts, centres, frames = ani.rdf_read()
    assert np.array_equal(counts[0], c.counts[3 * 4 + 0]) and np.array_equal(counts[1], c.counts[0 * 4 + 3])
    assert centres.tolist() == [168, 139] and frames == 1
    ani.close()
    # a half-list handle
    half = hx.decompose(rr.random_system(), half=True)
    ani = make(hip, model_cache, use_fullnbr=False)
    ani.compute(half, ago=0)
    p = np.zeros((1, 2), dtype=np.int32)
    rc = ani._lib.ani_rdf_configure(ani._h, 64, C.c_double(5.1), p.ctypes.data, 1)
    assert rc == ANI_ERR_ARG and b"half" in ani._lib.ani_last_error(ani._h)
    rc, msg = acc(ani, half.ntotal, half.nlocal)
    assert rc == ANI_ERR_ARG and "half" in msg
    ani.close()
