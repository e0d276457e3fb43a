"""GPU, no model: the kernels of include/ani_md_protocol.h through ani_hip.lib() on torch tensors, against the NumPy references of
tests/protocol_reference.py.

Random positions in the box of tests/transport_reference.py, image flags within +-3, masses of H, C, N, O, gaussian velocities with a
drift and a rotation added; every periodic mask, image flags given and NULL, the box on the host and on the device.  The bars are
protocol_reference.com_bounds / residual_bounds, from the sums of magnitudes.  n = 66 000 gives every finish more than 256 partials.
Every tensor that a kernel reads is held in a local until the call has been synchronised.
"""
import numpy as np
import pytest

import protocol_reference as pr
import transport_reference as tr
from test_md_loop_kernels import Device, U, _ptr, _same

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1000, 66000]
MASSES = np.array([1.008, 12.011, 14.007, 15.999])


@pytest.fixture(scope="module")
def dev():
    from lammps_ani_amd import ani_hip
    return Device(ani_hip)


def test_nothing_to_do_launches_nothing(dev):
    rng = np.random.default_rng(3)
    x, v, m, rec = rng.random((4, 3)), rng.random((4, 3)), rng.random(4) + 1.0, np.full(pr.COM_NREC, -1.0)
    t = [dev.up(a) for a in (x, v, m, rec, x + 0.1, np.full(17, -2.0))]
    d = dev.up(np.array([0.25]))
    for n in (0, -3):
        assert dev.lib.ani_md_com_sample(t[0].data_ptr(), None, t[1].data_ptr(), t[2].data_ptr(), n, tr.BOX_LO.ctypes.data,
                                         tr.BOX_LEN.ctypes.data, None, 7, t[5].data_ptr(), t[3].data_ptr(), None) == 0
        assert dev.lib.ani_md_com_apply(t[0].data_ptr(), t[1].data_ptr(), None, n, t[3].data_ptr(), 7, tr.BOX_LO.ctypes.data, 7,
                                        tr.BOX_LEN.ctypes.data, None, 7, t[4].data_ptr(), d.data_ptr(), None) == 0
    assert dev.lib.ani_md_com_apply(t[0].data_ptr(), t[1].data_ptr(), None, 4, t[3].data_ptr(), 0, None, 0, tr.BOX_LEN.ctypes.data, None, 7,
                                    t[4].data_ptr(), d.data_ptr(), None) == 0                       # no flag: nothing to apply
    x1, v1, rec1, work1, dd = dev.down(t[0], t[1], t[3], t[5], d)
    _same(x1, x, "x")
    _same(v1, v, "v")
    _same(rec1, rec, "record")
    _same(work1, np.full(17, -2.0), "scratch")
    assert dd[0] == 0.25 and dev.lib.ani_md_com_work_size(0) == 17 and dev.lib.ani_md_com_work_size(257) == 34


# ---- centre of mass ---------------------------------------------------------------------------------------------------------
def _atoms(n, seed):
    rng = np.random.default_rng(seed)
    x = tr.BOX_LO + tr.BOX_LEN * rng.random((n, 3))
    image = rng.integers(-3, 4, size=(n, 3)).astype(np.int32)
    m = rng.choice(MASSES, size=n)
    v = rng.normal(size=(n, 3)) * np.sqrt(pr.BOLTZ * 300.0 / (m[:, None] * pr.MVV2E))
    v += np.array([0.01, -0.02, 0.005]) + pr._cross(np.array([1e-3, -2e-3, 5e-4]), x - tr.BOX_LO)
    return x, image, v, m


def _sample(dev, x, image, v, m, mask, box_on_device=False):
    n = x.shape[0]
    L = tr.BOX_LEN.copy()
    ref = tr.BOX_LO + 0.5 * L
    t = [dev.up(a) for a in (x, v, m)]
    ti = None if image is None else dev.up(image)
    box = dev.up(L) if box_on_device else None
    work = dev.up(np.full(dev.lib.ani_md_com_work_size(n), np.nan))
    recs = []
    for _ in range(2):
        rec = dev.up(np.full(pr.COM_NREC, -1.0))
        assert dev.lib.ani_md_com_sample(t[0].data_ptr(), _ptr(ti), t[1].data_ptr(), t[2].data_ptr(), n, ref.ctypes.data,
                                         None if box_on_device else L.ctypes.data, _ptr(box), mask, work.data_ptr(), rec.data_ptr(), None) == 0
        recs.append(dev.down(rec)[0])
    assert recs[0].tobytes() == recs[1].tobytes()                               # no atomics: bitwise the same twice
    return recs[0], ref, L


FIELDS = (("mass", slice(0, 1)), ("xcm", slice(1, 4)), ("vcm", slice(4, 7)), ("angmom", slice(7, 10)), ("inertia", slice(10, 16)))


def _check_record(got, ref_rec, terms, what):
    bound = pr.com_bounds(ref_rec, terms)
    worst = 0.0
    for name, at in FIELDS:
        err = np.abs(got[at] - ref_rec[at])
        worst = max(worst, float((err / bound[name]).max()))
        assert (err <= bound[name]).all(), (what, name, err, bound[name])
    # omega solves I omega = L: through the tensor's condition number, on top of the bounds of its inputs
    I6 = ref_rec[pr.C_INERTIA:pr.C_INERTIA + 6]
    if not ref_rec[pr.C_SINGULAR]:
        I = np.array([[I6[0], I6[3], I6[4]], [I6[3], I6[1], I6[5]], [I6[4], I6[5], I6[2]]])
        w = ref_rec[pr.C_OMEGA:pr.C_OMEGA + 3]
        cond = np.linalg.cond(I)
        rel = cond * (bound["angmom"].max() / np.abs(ref_rec[pr.C_ANGMOM:pr.C_ANGMOM + 3]).max() + 3.0 * bound["inertia"].max() / np.abs(I).max()
                      + 64.0 * U)
        assert np.abs(got[pr.C_OMEGA:pr.C_OMEGA + 3] - w).max() <= rel * np.abs(w).max(), (what, cond)
    assert got[pr.C_SINGULAR] == ref_rec[pr.C_SINGULAR] and got[pr.C_NONFINITE] == ref_rec[pr.C_NONFINITE]
    assert got[pr.C_COUNT] == ref_rec[pr.C_COUNT] and (got[22:] == 0).all()
    return worst, got.tobytes() == ref_rec.tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_com_sample(n, dev):
    x, image, v, m = _atoms(n, 500 + n)
    for mask in range(8):
        for img in (image, None):
            got, ref, L = _sample(dev, x, img, v, m, mask, box_on_device=(mask == 5))
            want, terms = pr.com_sample(x, img, v, m, ref, L, mask)
            worst, same = _check_record(got, want, terms, (n, mask, img is None))
            if mask in (0, 7):
                print(f"  n = {n} mask {mask} image {'NULL' if img is None else 'given'}: largest error / bound {worst:.3f}, bitwise {same}")
    if n == 1:
        assert got[pr.C_SINGULAR] == 1 and (got[pr.C_OMEGA:pr.C_OMEGA + 3] == 0).all()


def test_com_sample_singular_and_nonfinite(dev):
    line = np.array([0.3, -0.5, 0.8])[None, :] * np.array([-1.0, 0.25, 2.0])[:, None] + np.array([2.0, 3.0, 5.0])
    v = np.random.default_rng(3).normal(size=(3, 3)) * 0.01
    m = np.array([1.008, 15.999, 1.008])
    got, ref, L = _sample(dev, line, None, v, m, 7)
    assert got[pr.C_SINGULAR] == 1 and (got[pr.C_OMEGA:pr.C_OMEGA + 3] == 0).all() and np.abs(got[pr.C_ANGMOM:pr.C_ANGMOM + 3]).max() > 0
    x, image, v, m = _atoms(600, 1)
    v[300, 1] = np.nan
    x[599, 2] = np.inf
    got, ref, L = _sample(dev, x, image, v, m, 7)
    assert got[pr.C_NONFINITE] == 2 and got[pr.C_COUNT] == 600
    # a record with NONFINITE != 0 applies nothing
    x, image, v, m = _atoms(600, 2)
    t = [dev.up(a) for a in (x, v, image, got, x + 0.1)]
    d = dev.up(np.array([0.0]))
    target = tr.BOX_LO + 0.5 * tr.BOX_LEN
    assert dev.lib.ani_md_com_apply(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 600, t[3].data_ptr(), 7, target.ctypes.data, 7,
                                    tr.BOX_LEN.ctypes.data, None, 7, t[4].data_ptr(), d.data_ptr(), None) == 0
    x1, v1, d1 = dev.down(t[0], t[1], d)
    _same(x1, x, "x under a non-finite record")
    _same(v1, v, "v under a non-finite record")
    assert d1[0] == 0.0


@pytest.mark.parametrize("n", SIZES)
def test_com_apply(n, dev):
    x, image, v, m = _atoms(n, 900 + n)
    xb = x + np.random.default_rng(n).normal(0.0, 0.05, (n, 3))
    target = tr.BOX_LO + np.array([0.5, 0.25, 0.75]) * tr.BOX_LEN
    for mask, img in ((7, image), (5, image), (7, None)):
        rec, ref, L = _sample(dev, x, img, v, m, mask)
        _, terms = pr.com_sample(x, img, v, m, ref, L, mask)
        for flags in range(1, 8):
            dim_mask = 0b101 if flags == 4 else 7
            t = [dev.up(a) for a in (x, v, rec, xb)]
            ti = None if img is None else dev.up(img)
            d = dev.up(np.array([0.0]))
            assert dev.lib.ani_md_com_apply(t[0].data_ptr(), t[1].data_ptr(), _ptr(ti), n, t[2].data_ptr(), flags, target.ctypes.data,
                                            dim_mask, L.ctypes.data, None, mask, t[3].data_ptr(), d.data_ptr(), None) == 0
            x1, v1, d1 = dev.down(t[0], t[1], d)
            xr, vr, dr = pr.com_apply(x, v, img, rec, flags, target, dim_mask, L, mask, x_built=xb, d2max=0.0)
            # the apply rounds every operation on its own, as the reference does, from the same record: a few roundings of slack
            r = np.abs(pr._unwrapped(x, img, L, mask) - rec[pr.C_XCM:pr.C_XCM + 3])
            w = np.abs(rec[pr.C_OMEGA:pr.C_OMEGA + 3])
            mv = np.abs(v) + np.abs(rec[pr.C_VCM:pr.C_VCM + 3]) + 2.0 * np.abs(pr._cross(w, r)) + w.max() * r.sum(1, keepdims=True)
            assert (np.abs(v1 - vr) <= 8.0 * U * mv).all(), (n, mask, flags)
            assert (np.abs(x1 - xr) <= 4.0 * U * (np.abs(x) + np.abs(target) + np.abs(rec[pr.C_XCM:pr.C_XCM + 3]))).all(), (n, mask, flags)
            same = x1.tobytes() == xr.tobytes() and v1.tobytes() == vr.tobytes()
            if not flags & 4:
                _same(x1, x, "x without the recentre bit")
                assert d1[0] == 0.0
            else:
                assert abs(d1[0] - dr) <= 32.0 * U * max(dr, 1.0)
            if not flags & 3:
                _same(v1, v, "v without a momentum bit")
            # the reference's own sample of the downloaded arrays: what was to be removed is gone, to the bounds
            rec1, terms1 = pr.com_sample(x1, img, v1, m, ref, L, mask)
            bound = pr.residual_bounds(rec, rec1, terms, terms1, flags & 1, flags & 2 and n > 2)
            if flags & 1:
                P = rec1[pr.C_MASS] * np.abs(rec1[pr.C_VCM:pr.C_VCM + 3])
                assert (P <= bound["P"]).all(), (n, mask, flags, P, bound["P"])
            if flags & 2 and n > 2:
                Lr = np.abs(rec1[pr.C_ANGMOM:pr.C_ANGMOM + 3])
                assert (Lr <= bound["L"]).all(), (n, mask, flags, Lr, bound["L"])
            if flags & 4:
                b = pr.com_bounds(rec, terms)["xcm"] + pr.com_bounds(rec1, terms1)["xcm"] + 4.0 * U * np.abs(x1).max()
                off = np.abs(rec1[pr.C_XCM:pr.C_XCM + 3] - target)
                dims = [k for k in range(3) if (dim_mask >> k) & 1]
                assert (off[dims] <= b[dims]).all(), (n, mask, flags, off, b)
        print(f"  n = {n} mask {mask} image {'NULL' if img is None else 'given'}: last apply bitwise the reference's: {same}")
