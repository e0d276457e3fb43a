"""GPU, no model: the kernels of include/ani_md_transport.h through ani_hip.lib() on torch tensors, against the NumPy references
of tests/transport_reference.py.

Wrap: 3 n elements in blocks of 256, so n = 85 and 86 straddle one block; box lo (-1.5, 0, 2), len (8, 9.5, 11); random coordinates
within +-3 box lengths and the edge list (exactly lo, exactly lo + L, lo - 1e-17, the double under lo + L, lo -+ 3 L) in every
dimension.  x bitwise as ani_md_wrap_positions leaves a copy, image as the reference's rule gives it.
MSD: n = 66 000 gives the finish kernel more than 256 partials per sum.  The rounding bound is derived in
transport_reference.msd_bounds.  Frame pack: bitwise against np.float32 of the reference.
"""
import numpy as np
import pytest

import transport_reference as tr

pytestmark = pytest.mark.gpu

SIZES_WRAP = [1, 85, 86, 256, 257, 1000]
SIZES = [1, 255, 256, 257, 1000, 66000]
GROUP_MASKS = np.array([0b111, 0b010, 0b101, 0], dtype=np.int32)      # all classes; one class; two classes; an empty group


@pytest.fixture(scope="module")
def dev():
    import torch
    from lammps_ani_amd import ani_hip

    class Dev:
        lib = ani_hip.lib()
        device = torch.device("cuda:0")

        def put(self, a):
            return torch.as_tensor(np.ascontiguousarray(a), device=self.device)

        def sync(self):
            torch.cuda.synchronize()
    return Dev()


def _wrap_both(dev, x0, img0, mask):
    lo, L = tr.BOX_LO.copy(), tr.BOX_LEN.copy()
    n = x0.shape[0]
    tx, tplain, timg = dev.put(x0), dev.put(x0), dev.put(img0)
    assert dev.lib.ani_md_wrap_positions(tplain.data_ptr(), n, lo.ctypes.data, L.ctypes.data, mask, None) == 0
    assert dev.lib.ani_md_wrap_positions_images(tx.data_ptr(), timg.data_ptr(), n, lo.ctypes.data, L.ctypes.data, mask, None) == 0
    dev.sync()
    x1, img1 = tx.cpu().numpy(), timg.cpu().numpy()
    assert x1.tobytes() == tplain.cpu().numpy().tobytes()
    xr, imgr = tr.wrap_images(x0, img0, lo, L, mask)
    assert (img1 == imgr).all(), np.argwhere(img1 != imgr)[:5]
    assert dev.lib.ani_md_wrap_positions_images(tx.data_ptr(), timg.data_ptr(), n, lo.ctypes.data, L.ctypes.data, mask, None) == 0
    dev.sync()
    assert tx.cpu().numpy().tobytes() == x1.tobytes() and (timg.cpu().numpy() == img1).all()      # a second call adds nothing
    return x1, img1, xr


@pytest.mark.parametrize("n", SIZES_WRAP)
def test_wrap_positions_images(n, dev):
    rng = np.random.default_rng(100 + n)
    agree = 0
    for mask in range(8):
        starts = [tr.wrap_coordinates(n, 7 * n + mask)]
        if n == 1:
            starts = [e[None, :].copy() for e in tr.wrap_edges()]          # one atom: every edge value in its own call
        for x0 in starts:
            img0 = rng.integers(-5, 6, size=x0.shape).astype(np.int32)
            x1, img1, xr = _wrap_both(dev, x0, img0, mask)
            agree += int(x1.tobytes() == xr.tobytes())
            for k in range(3):
                if not (mask >> k) & 1:
                    assert (x1[:, k] == x0[:, k]).all() and (img1[:, k] == img0[:, k]).all()
                else:
                    assert (x1[:, k] >= tr.BOX_LO[k]).all() and (x1[:, k] < tr.BOX_LO[k] + tr.BOX_LEN[k]).all()
    print(f"n = {n}: x also bitwise the plain fp64 reference's in {agree} calls")


def test_wrap_with_nothing_to_do_leaves_both_arrays(dev):
    lo, L = tr.BOX_LO.copy(), tr.BOX_LEN.copy()
    x0 = tr.wrap_coordinates(300, 1)
    img0 = np.full(x0.shape, 3, dtype=np.int32)
    tx, timg = dev.put(x0), dev.put(img0)
    assert dev.lib.ani_md_wrap_positions_images(tx.data_ptr(), timg.data_ptr(), 300, lo.ctypes.data, L.ctypes.data, 0, None) == 0
    assert dev.lib.ani_md_wrap_positions_images(tx.data_ptr(), timg.data_ptr(), 0, lo.ctypes.data, L.ctypes.data, 7, None) == 0
    dev.sync()
    assert tx.cpu().numpy().tobytes() == x0.tobytes() and (timg.cpu().numpy() == img0).all()


def _msd_case(n):
    rng = np.random.default_rng(4000 + n)
    L = tr.BOX_LEN
    x = tr.BOX_LO + L * rng.random((n, 3))
    img = rng.integers(-1000, 1001, size=(n, 3)).astype(np.int32)
    cls = rng.integers(-1, 3, size=n).astype(np.int32)
    cls[0] = 0                                       # the one atom of the smallest size is in a group
    mass = rng.choice([1.008, 15.999], size=n)
    x0u = tr.unwrap(x, img, L, 7) + rng.normal(size=(n, 3)) * 3.0 + np.array([0.7, -0.4, 0.2])
    return x, img, cls, mass, x0u


def _msd_call(dev, x, img, cls, mass, x0u, mask, box_on_device, step=17.0):
    from lammps_ani_amd import ani_hip
    n, L, ng = x.shape[0], tr.BOX_LEN.copy(), len(GROUP_MASKS)
    count = np.array([(cls == c).sum() for c in range(3)], dtype=np.int32)
    cmass = np.array([mass[cls == c].sum() for c in range(3)])
    t = [dev.put(a) for a in (x, img, x0u, mass, cls, count, cmass, GROUP_MASKS)]
    box = dev.put(L) if box_on_device else None
    work = dev.put(np.full(dev.lib.ani_md_msd_work_size(n, 3), np.nan))          # scratch needs no initialisation
    outs = []
    for _ in range(2):
        out, row = dev.put(np.full((ng, ani_hip.MSD_NOUT), -1.0)), dev.put(np.full(1 + ng * ani_hip.MSD_NOUT, -1.0))
        rc = dev.lib.ani_md_msd_sample(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), n, 3,
                                       t[5].data_ptr(), t[6].data_ptr(), t[7].data_ptr(), ng, None if box_on_device else L.ctypes.data,
                                       box.data_ptr() if box_on_device else None, mask, work.data_ptr(), out.data_ptr(), step,
                                       row.data_ptr(), None)
        assert rc == 0
        dev.sync()
        outs.append((out.cpu().numpy(), row.cpu().numpy()))
    (o1, r1), (o2, r2) = outs
    assert o1.tobytes() == o2.tobytes() and r1.tobytes() == r2.tobytes()         # no atomics: bitwise the same twice
    assert r1[0] == step and r1[1:].tobytes() == o1.tobytes()
    return o1


@pytest.mark.parametrize("box_on_device", [False, True], ids=["len3", "box_dev"])
@pytest.mark.parametrize("n", SIZES)
def test_msd_sample(n, box_on_device, dev):
    x, img, cls, mass, x0u = _msd_case(n)
    mask = 7 if n != 257 else 5                      # one size with a non-periodic dimension: its image is not applied
    out = _msd_call(dev, x, img, cls, mass, x0u, mask, box_on_device)
    xu = tr.unwrap(x, img, tr.BOX_LEN, mask)
    worst = 0.0
    for g, gm in enumerate(GROUP_MASKS):
        members = np.array([(c >= 0) and bool((gm >> c) & 1) for c in cls.tolist()], dtype=bool)
        ref, terms = tr.msd(xu, x0u, mass, members)
        bound = tr.msd_bounds(terms)
        err = np.abs(out[g] - ref)
        print(f"n = {n} group {g} (N = {terms['N']}): |error| {np.array2string(err, precision=2)}\n    bound  "
              f"{np.array2string(bound, precision=2)}")
        assert np.isfinite(out[g]).all() and (err <= bound).all(), (g, err, bound)
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    assert not out[3].any()                                                       # the empty group is all zeros
    print(f"n = {n}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("n", SIZES)
def test_msd_one_nan_position_reaches_exactly_its_groups(n, dev):
    x, img, cls, mass, x0u = _msd_case(n)
    i = n // 2
    cls[i] = 1
    clean = _msd_call(dev, x, img, cls, mass, x0u, 7, False)
    x[i] = np.nan
    out = _msd_call(dev, x, img, cls, mass, x0u, 7, False)
    for g in (0, 1):                                                              # all classes, and class 1 alone
        assert np.isnan(out[g, :11]).all() and out[g, 11] == 1.0
    assert np.isfinite(out[2]).all() and out[2, 11] == 0.0 and out[2].tobytes() == clean[2].tobytes()    # classes 0 and 2
    assert not out[3].any()


@pytest.mark.parametrize("unwrap", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_frame_pack(n, unwrap, dev):
    rng = np.random.default_rng(9000 + n)
    lo, L = tr.BOX_LO.copy(), tr.BOX_LEN.copy()
    x = lo + L * rng.random((n, 3))
    img = rng.integers(-1000, 1001, size=(n, 3)).astype(np.int32)
    row = rng.permutation(n).astype(np.int32)
    src = tr.unwrap(x, img, L, 7) if unwrap else x
    want = np.zeros((3, n), dtype=np.float32)
    want[:, row] = np.float32(src).T
    tx, timg = dev.put(x), dev.put(img)
    lo_d, len_d = dev.put(lo + 0.25), dev.put(L)                                  # the device record's lo differs from the host's

    def pack(rows, on_device):
        xyz, cell = dev.put(np.full((3, n), 777.0, dtype=np.float32)), dev.put(np.full(6, -1.0))
        rc = dev.lib.ani_md_frame_pack(tx.data_ptr(), timg.data_ptr() if unwrap else None, n, dev.put(rows).data_ptr(), lo.ctypes.data,
                                       None if on_device else L.ctypes.data, lo_d.data_ptr() if on_device else None,
                                       len_d.data_ptr() if on_device else None, 7, unwrap, xyz.data_ptr(), cell.data_ptr(), None)
        assert rc == 0
        dev.sync()
        return xyz.cpu().numpy(), cell.cpu().numpy()

    for on_device in (False, True):
        xyz, cell = pack(row, on_device)
        assert xyz.tobytes() == want.tobytes()
        assert cell.tobytes() == np.concatenate([lo + 0.25 if on_device else lo, L]).tobytes()
    # one row that points outside: its atom is skipped, its place in the frame is never written, every other row is right
    bad = row.copy()
    i = n // 3
    bad[i] = n
    xyz, _ = pack(bad, False)
    hole = want.copy()
    hole[:, row[i]] = 777.0
    assert xyz.tobytes() == hole.tobytes()
    bad[i] = -1
    assert pack(bad, False)[0].tobytes() == hole.tobytes()


def test_unwrap_is_the_definition(dev):
    n = 1000
    rng = np.random.default_rng(77)
    L = np.array([9.3217, 8.1113, 10.777])                                        # products that round
    x = rng.uniform(-1.0, 11.0, size=(n, 3))
    img = rng.integers(-1000, 1001, size=(n, 3)).astype(np.int32)
    tx, timg, box = dev.put(x), dev.put(img), dev.put(L)
    for mask in (7, 2, 0):
        for on_device in (False, True):
            out = dev.put(np.zeros((n, 3)))
            assert dev.lib.ani_md_unwrap(tx.data_ptr(), timg.data_ptr(), n, None if on_device else L.ctypes.data,
                                         box.data_ptr() if on_device else None, mask, out.data_ptr(), None) == 0
            dev.sync()
            assert out.cpu().numpy().tobytes() == tr.unwrap(x, img, L, mask).tobytes()


def test_refusals(dev):
    z = dev.put(np.zeros(64))
    p = z.data_ptr()
    L = tr.BOX_LEN.copy()
    args = lambda nclass, ngroup: (p, p, p, p, p, 4, nclass, p, p, p, ngroup, L.ctypes.data, None, 7, p, p, 0.0, None, None)   # noqa: E731
    for nclass, ngroup in ((0, 1), (17, 1), (1, 0), (1, 9)):
        assert dev.lib.ani_md_msd_sample(*args(nclass, ngroup)) != 0
    assert dev.lib.ani_md_msd_work_size(1000, 3) >= 3 * 10 * 4
