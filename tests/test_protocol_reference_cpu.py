"""CPU: tests/protocol_reference.py on its own -- what the momentum removal leaves and takes, the singular cases, recentring and the
independence of the record from the reference point -- and the record layout of include/ani_md_protocol.h against the table of
ani_hip.py."""
import os
import re

import numpy as np

import protocol_reference as pr
import transport_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASSES = np.array([1.008, 12.011, 14.007, 15.999])


def _atoms(n, seed):
    rng = np.random.default_rng(seed)
    x = tr.BOX_LO + tr.BOX_LEN * rng.random((n, 3))
    image = rng.integers(-3, 4, size=(n, 3)).astype(np.int32)
    m = rng.choice(MASSES, size=n)
    v = rng.normal(size=(n, 3)) * np.sqrt(pr.BOLTZ * 300.0 / (m[:, None] * pr.MVV2E))
    return x, image, v, m


def test_record_layout_of_ani_md_protocol_h_and_ani_hip_py_agree():
    """as tests/test_abi_exports.py does for include/ani_md.h: same fields, same first words, a field of several words ends where
    the next begins, the counts agree; and this file's reference uses the same offsets"""
    from lammps_ani_amd import ani_hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ani_md_protocol.h")).read(), flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(ANI_MD_\w+)\s+(\d+)\s*$", hdr, flags=re.M)}
    members = {}
    for body in re.findall(r"\benum\s*\{(.*?)\}", hdr, flags=re.S):
        value = -1
        for item in filter(None, (s.strip() for s in body.split(","))):
            name, _, given = (s.strip() for s in item.partition("="))
            value = int(given) if given else value + 1
            assert name not in members and name not in defines, name
            members[name] = value
    records = {"ANI_MD_COM_": (ani_hip.COM_LAYOUT, "ANI_MD_COM_NREC")}
    assert all(any(name.startswith(p) for p in records) for name in members), sorted(members)
    for prefix, (table, count) in records.items():
        in_header = sorted((v, k[len(prefix):]) for k, v in members.items() if k.startswith(prefix))
        starts = {k.upper(): (at.start if isinstance(at, slice) else at) for k, at in table.items()}
        assert len(starts) == len(table) and starts == {k: v for v, k in in_header}, prefix
        ends = [v for v, _ in in_header[1:]] + [defines[count]]
        for (first, name), end in zip(in_header, ends):
            at = {k.upper(): at for k, at in table.items()}[name]
            assert first < end <= defines[count], (prefix, name)
            assert (at.stop, at.step) == (end, None) if isinstance(at, slice) else end == first + 1, (prefix, name)
    assert ani_hip.COM_NREC == defines["ANI_MD_COM_NREC"] == pr.COM_NREC
    assert (ani_hip.COM_FLAG_LINEAR, ani_hip.COM_FLAG_ANGULAR, ani_hip.COM_FLAG_RECENTER) == tuple(
        defines["ANI_MD_COM_FLAG_" + k] for k in ("LINEAR", "ANGULAR", "RECENTER"))
    Cm = ani_hip.COM_LAYOUT
    assert [Cm[k].start for k in ("xcm", "vcm", "angmom", "inertia", "omega")] + [Cm[k] for k in ("mass", "singular", "nonfinite", "count")] \
        == [pr.C_XCM, pr.C_VCM, pr.C_ANGMOM, pr.C_INERTIA, pr.C_OMEGA, pr.C_MASS, pr.C_SINGULAR, pr.C_NONFINITE, pr.C_COUNT]


def test_block_sums_and_finish_add_everything_once():
    rng = np.random.default_rng(5)
    for n in (1, 255, 256, 257, 1000, 66000):
        a = rng.integers(-1000, 1000, size=n).astype(np.float64)            # integers: every order gives the same sum exactly
        part = pr.block_sums(a)
        assert part.shape == ((n + 255) // 256,) and part.sum() == a.sum() and pr.finish(part) == a.sum()


def test_momentum_removal_leaves_zero_and_takes_the_rigid_body_energy():
    L = tr.BOX_LEN
    ref = tr.BOX_LO + 0.5 * L
    for n in (2, 3, 30, 1000):
        x, image, v, m = _atoms(n, 20 + n)
        v = v + np.array([0.01, -0.02, 0.005]) + pr._cross(np.array([1e-3, -2e-3, 5e-4]), pr._unwrapped(x, image, L, 7) - ref)
        rec, terms = pr.com_sample(x, image, v, m, ref, L, 7)
        for flags in (1, 2, 3):
            if n == 2 and flags & 2:
                continue                                                    # two atoms are collinear: below
            _, v1, _ = pr.com_apply(x, v, image, rec, flags, None, 0, L, 7)
            rec1, terms1 = pr.com_sample(x, image, v1, m, ref, L, 7)
            bound = pr.residual_bounds(rec, rec1, terms, terms1, flags & 1, flags & 2)
            if flags & 1:
                P = rec1[pr.C_MASS] * np.abs(rec1[pr.C_VCM:pr.C_VCM + 3])
                assert (P <= bound["P"]).all(), (n, flags, P, bound["P"])
            if flags & 2:
                Lr = np.abs(rec1[pr.C_ANGMOM:pr.C_ANGMOM + 3])
                assert (Lr <= bound["L"]).all(), (n, flags, Lr, bound["L"])
                assert np.abs(rec[pr.C_ANGMOM:pr.C_ANGMOM + 3]).min() > 1e6 * bound["L"].max()      # there was something to remove
            # the kinetic energy falls by the rigid-body part: 1/2 M VCM^2 (linear) + 1/2 omega . L (angular)
            vcm, w, ang = rec[pr.C_VCM:pr.C_VCM + 3], rec[pr.C_OMEGA:pr.C_OMEGA + 3], rec[pr.C_ANGMOM:pr.C_ANGMOM + 3]
            want = 0.5 * pr.MVV2E * ((rec[pr.C_MASS] * (vcm * vcm).sum() if flags & 1 else 0.0) + ((w * ang).sum() if flags & 2 else 0.0))
            fell = pr.kinetic(m, v) - pr.kinetic(m, v1)
            assert abs(fell - want) <= (n / 256.0 + 64.0) * 8.0 * pr.EPS * pr.kinetic(m, np.abs(v)), (n, flags, fell, want)
            assert want > 0.0


def test_singular_inertia_gives_zero_omega():
    L, ref = tr.BOX_LEN, tr.BOX_LO + 0.5 * tr.BOX_LEN
    one = pr.com_sample(np.array([[1.0, 2.0, 3.0]]), None, np.array([[0.1, 0.2, 0.3]]), np.array([12.011]), ref, L, 7)[0]
    assert one[pr.C_SINGULAR] == 1 and (one[pr.C_OMEGA:pr.C_OMEGA + 3] == 0).all() and one[pr.C_COUNT] == 1
    assert np.allclose(one[pr.C_XCM:pr.C_XCM + 3], [1.0, 2.0, 3.0], rtol=0, atol=1e-14)
    line = np.array([0.3, -0.5, 0.8])[None, :] * np.array([-1.0, 0.25, 2.0])[:, None] + np.array([2.0, 3.0, 5.0])
    v = np.random.default_rng(3).normal(size=(3, 3)) * 0.01
    rec = pr.com_sample(line, None, v, np.array([1.008, 15.999, 1.008]), ref, L, 7)[0]
    assert rec[pr.C_SINGULAR] == 1 and (rec[pr.C_OMEGA:pr.C_OMEGA + 3] == 0).all()
    assert np.abs(rec[pr.C_ANGMOM:pr.C_ANGMOM + 3]).max() > 0                  # the angular momentum itself is reported
    x1, v1, _ = pr.com_apply(line, v, None, rec, 2, None, 0, L, 7)
    assert (v1 == v).all() and (x1 == line).all()
    bent = line.copy()
    bent[1] += np.array([0.0, 0.4, 0.0])
    assert pr.com_sample(bent, None, v, np.array([1.008, 15.999, 1.008]), ref, L, 7)[0][pr.C_SINGULAR] == 0


def test_record_does_not_depend_on_the_reference_point_beyond_its_bound():
    L, ref = tr.BOX_LEN, tr.BOX_LO + 0.5 * tr.BOX_LEN
    for n in (30, 1000):
        x, image, v, m = _atoms(n, 40 + n)
        a, ta = pr.com_sample(x, image, v, m, ref, L, 7)
        b, tb = pr.com_sample(x, image, v, m, ref + L, L, 7)
        ba, bb = pr.com_bounds(a, ta), pr.com_bounds(b, tb)
        for name, at in (("xcm", slice(pr.C_XCM, pr.C_XCM + 3)), ("inertia", slice(pr.C_INERTIA, pr.C_INERTIA + 6))):
            err = np.abs(a[at] - b[at])
            print(f"n = {n} {name}: largest |difference| / bound {(err / (ba[name] + bb[name])).max():.3f}")
            assert (err <= ba[name] + bb[name]).all(), (name, err, ba[name] + bb[name])
        far = pr.com_bounds(*pr.com_sample(x, image, v, m, ref + 100.0 * L, L, 7))
        assert (far["inertia"] > 100.0 * ba["inertia"]).all()                # a far reference pays for the parallel-axis shift


def test_recenter_puts_the_centre_of_mass_on_the_target():
    L, ref = tr.BOX_LEN, tr.BOX_LO + 0.5 * tr.BOX_LEN
    x, image, v, m = _atoms(300, 9)
    rec, terms = pr.com_sample(x, image, v, m, ref, L, 5)
    target = tr.BOX_LO + np.array([0.5, 0.25, 0.75]) * L
    x1, v1, d2 = pr.com_apply(x, v, image, rec, 4, target, 0b101, L, 5, x_built=x, d2max=0.0)
    rec1, terms1 = pr.com_sample(x1, image, v1, m, ref, L, 5)
    bound = pr.com_bounds(rec, terms)["xcm"] + pr.com_bounds(rec1, terms1)["xcm"] + 4 * pr.EPS * np.abs(x1).max()
    off = np.abs(rec1[pr.C_XCM:pr.C_XCM + 3] - target)
    assert (off[[0, 2]] <= bound[[0, 2]]).all() and (x1[:, 1] == x[:, 1]).all() and (v1 == v).all()
    shift = target - rec[pr.C_XCM:pr.C_XCM + 3]
    assert abs(d2 - (shift[0] ** 2 + shift[2] ** 2)) <= 1e-12 * d2
    nan = rec.copy()
    nan[pr.C_NONFINITE] = 1.0
    x2, v2, d2 = pr.com_apply(x, v, image, nan, 7, target, 7, L, 5, x_built=x, d2max=0.25)
    assert (x2 == x).all() and (v2 == v).all() and d2 == 0.25
