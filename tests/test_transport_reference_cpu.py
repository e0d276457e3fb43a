"""CPU: the NumPy references of tests/transport_reference.py against what they stand for, and the DCD writer of
lammps-ani_amd/dcd.py against the reader written from its format description."""
import os
import struct

import numpy as np
import pytest

import transport_reference as tr


@pytest.mark.parametrize("mask", range(8))
def test_wrap_images_keeps_the_unwrapped_coordinate(mask):
    """x + image L after the wrap is the coordinate before it, within 2 ulp of max(|x_old|, |q| L) (the product q L, the difference
    and the sum round once each at that magnitude), on random coordinates and the edge list; every wrapped coordinate lies in
    [lo, lo + L); non-periodic components are untouched; a second wrap adds nothing."""
    lo, L = tr.BOX_LO, tr.BOX_LEN
    x0 = np.concatenate([tr.wrap_coordinates(500, 11), tr.wrap_edges()])
    img0 = np.random.default_rng(5).integers(-4, 5, size=x0.shape).astype(np.int32)
    x1, img1 = tr.wrap_images(x0, img0, lo, L, mask)
    for k in range(3):
        if not (mask >> k) & 1:
            assert (x1[:, k] == x0[:, k]).all() and (img1[:, k] == img0[:, k]).all()
            continue
        assert (x1[:, k] >= lo[k]).all() and (x1[:, k] < lo[k] + L[k]).all()
        q = (img1[:, k] - img0[:, k]).astype(np.float64)
        back = x1[:, k] + q * L[k]
        floor_q = np.floor((x0[:, k] - lo[k]) / L[k])               # the q of the rule; the count added is q or q + 1
        assert ((q == floor_q) | (q == floor_q + 1)).all()
        bar = 2.0 * np.spacing(np.maximum(np.abs(x0[:, k]), np.abs(floor_q) * L[k]))
        assert (np.abs(back - x0[:, k]) <= bar).all(), np.abs(back - x0[:, k]).max()
    assert np.abs(img1 - img0).max() <= (4 if mask else 0)
    x2, img2 = tr.wrap_images(x1, img1, lo, L, mask)
    assert x2.tobytes() == x1.tobytes() and (img2 == img1).all()
    xu = tr.unwrap(x1, img1 - img0, L, mask)
    assert np.abs(xu - x0).max() <= 2.0 * np.spacing(np.abs(x0).max() + 3.0 * L.max())


def test_wrap_images_at_the_faces():
    lo, L = tr.BOX_LO, tr.BOX_LEN
    e = tr.wrap_edges()
    x, img = tr.wrap_images(e, np.zeros(e.shape, np.int32), lo, L, 7)
    assert (x[0] == lo).all() and (img[0] == 0).all()                       # exactly lo stays
    assert (x[1] == lo).all() and (img[1] == 1).all()                       # exactly lo + L is lo of the next image
    assert (x[4] == lo).all() and (img[4] == -3).all() and (x[5] == lo).all() and (img[5] == 3).all()
    assert (x[3] >= lo).all() and (x[3] < lo + L).all() and set(img[3].tolist()) <= {0, 1}
    assert (np.abs(x[2] + img[2] * L - e[2]) <= 2.0 * np.spacing(np.maximum(np.abs(e[2]), L))).all()


def test_msd_reference_and_its_bound():
    """the direct form of the reference against the closed form of the header in plain fp64, inside the reference's own bound; an
    empty group is all zeros; a uniform translation has com-yes MSD zero within the bound"""
    rng = np.random.default_rng(3)
    n = 500
    x0u = rng.uniform(-20.0, 20.0, size=(n, 3))
    xu = x0u + rng.normal(size=(n, 3)) * 3.0 + np.array([4.0, -4.0, 4.0])
    mass = rng.choice([1.008, 15.999], size=n)
    sel = rng.random(n) < 0.6
    out, terms = tr.msd(xu, x0u, mass, sel)
    bound = tr.msd_bounds(terms)
    d, m = (xu - x0u)[sel], mass[sel]
    N, M = sel.sum(), m.sum()
    s2, s1, dcm = (d * d).sum(0) / N, d.sum(0) / N, (m[:, None] * d).sum(0) / M
    closed = np.concatenate([s2, [s2.sum()], s2 - 2 * dcm * s1 + dcm * dcm, [(s2 - 2 * dcm * s1 + dcm * dcm).sum()], dcm, [0.0]])
    assert (np.abs(closed - out) <= bound).all(), (np.abs(closed - out), bound)
    assert (bound[:11] > 0).all() and bound[11] == 0 and (bound[:11] < 1e-12).all()
    empty, terms0 = tr.msd(xu, x0u, mass, np.zeros(n, bool))
    assert not empty.any() and not tr.msd_bounds(terms0).any()
    shifted, terms1 = tr.msd(x0u + np.array([1.0, 2.0, -3.0]), x0u, mass, sel)
    assert (np.abs(shifted[4:8]) <= tr.msd_bounds(terms1)[4:8]).all() and np.allclose(shifted[8:11], [1.0, 2.0, -3.0], atol=1e-13)


@pytest.mark.parametrize("natoms", [1, 3, 30])
def test_dcd_round_trip(natoms, tmp_path):
    """writer -> reader bitwise; the file has 276 + nf (56 + 3 (4 N + 8)) bytes, and NSET and the last step are right after every
    append"""
    from lammps_ani_amd import dcd
    rng = np.random.default_rng(natoms)
    path = str(tmp_path / "t.dcd")
    first, every, dt = 40, 20, 0.5
    w = dcd.DCDWriter(path, natoms, first, every, dt)
    assert os.path.getsize(path) == 276 and tr.read_dcd(path)["nset"] == 0
    cells, blocks = [], []
    for f in range(4):
        cell = np.concatenate([rng.uniform(-2, 0, 3), rng.uniform(8, 12, 3)])
        block = rng.normal(size=(3, natoms)).astype(np.float32) * 10.0
        w.append(cell, block if f % 2 else block.tobytes())
        cells.append(cell)
        blocks.append(block)
        got = tr.read_dcd(path)
        assert got["size"] == os.path.getsize(path) == 276 + (f + 1) * (56 + 3 * (4 * natoms + 8)) == 276 + (f + 1) * dcd.frame_bytes(natoms)
        assert got["nset"] == f + 1 and got["last_step"] == first + f * every and got["first_step"] == first and got["every"] == every
        raw = open(path, "rb").read()
        assert struct.unpack_from("<i", raw, 8)[0] == f + 1 and struct.unpack_from("<i", raw, 20)[0] == first + f * every
    w.close()
    got = tr.read_dcd(path)
    assert got["natoms"] == natoms and got["dt"] == np.float32(dt) and all(len(r) == 80 for r in got["remarks"])
    assert got["cell"].tobytes() == np.array(cells)[:, 3:].tobytes() and not got["cosines"].any()
    assert got["xyz"].tobytes() == np.array(blocks).transpose(0, 2, 1).copy().tobytes()
    with pytest.raises(ValueError, match="closed"):
        w.append(cells[0], blocks[0])
    with pytest.raises(ValueError, match="bytes"):
        dcd.DCDWriter(str(tmp_path / "u.dcd"), natoms, 0, 1, dt).append(cells[0], np.zeros((3, natoms + 1), np.float32))


def test_msd_classes_are_the_membership_patterns():
    from lammps_ani_amd import ani_hip
    member = np.array([[1, 1, 1, 1, 0, 0], [0, 1, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0]], dtype=bool)
    cls, masks, nclass = ani_hip.msd_classes(member)
    assert nclass == 2 and cls.tolist() == [0, 1, 0, 1, -1, -1] and masks.tolist() == [0b11, 0b10, 0]
    assert ani_hip.MSD_LAYOUT["nonfinite"] + 1 == ani_hip.MSD_NOUT
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ani_md_transport.h")).read()
    for name, value in (("MAXCLASS", ani_hip.MSD_MAXCLASS), ("MAXGROUP", ani_hip.MSD_MAXGROUP), ("NOUT", ani_hip.MSD_NOUT)):
        assert f"#define ANI_MD_MSD_{name} {value}\n" in hdr
    for key, at in ani_hip.MSD_LAYOUT.items():
        start = at.start if isinstance(at, slice) else at
        assert f"ANI_MD_MSD_{'COM' if key == 'com' else key.upper()} = {start}" in hdr
