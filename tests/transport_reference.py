"""NumPy references for the kernels of include/ani_md_transport.h and a reader for the files of lammps-ani_amd/dcd.py, written
from the header's and the module's text, not from their code.

wrap_images   ani_md_wrap_positions_images: the rule of the header, literally, in plain double precision
unwrap        the unwrapped coordinate: x + float64(image) * len, product and sum rounded separately (which is what NumPy does)
msd           the MSD outputs in the direct form, mean |d - dcm|^2, with np.longdouble sums, and the absolute sums that the rounding
              bound of the tests is made of
msd_bounds    that bound
read_dcd      the DCD reader
"""
import struct

import numpy as np

NOUT = 12
EPS = 2.0 ** -53


BOX_LO = np.array([-1.5, 0.0, 2.0])
BOX_LEN = np.array([8.0, 9.5, 11.0])


def wrap_edges(lo=BOX_LO, length=BOX_LEN):
    """[7, 3]: in every dimension exactly lo, exactly lo + L, lo - 1e-17, the double just under lo + L, and lo -+ 3 L"""
    lo, length = np.asarray(lo, dtype=np.float64), np.asarray(length, dtype=np.float64)
    return np.stack([lo, lo + length, lo - 1e-17, np.nextafter(lo + length, -np.inf), lo - 3.0 * length, lo + 3.0 * length,
                     lo + 0.5 * length])[:7]


def wrap_coordinates(n, seed, lo=BOX_LO, length=BOX_LEN):
    """[n, 3] coordinates within +-3 box lengths of the box, the first rows (as many as fit) the edge list, each edge value
    standing in every dimension at once"""
    rng = np.random.default_rng(seed)
    x = lo + length * rng.uniform(-3.0, 4.0, size=(n, 3))
    e = wrap_edges(lo, length)
    x[: min(n, len(e))] = e[: min(n, len(e))]
    return x


def wrap_images(x, image, lo, length, mask):
    """(x, image) after the wrap.  Per periodic component: q = floor((v - lo) / L); v -= q L; image += q; where v >= lo + L: v = lo
    and image += 1 more; where then v < lo: v = lo."""
    x = np.array(x, dtype=np.float64)
    image = np.array(image, dtype=np.int32)
    for k in range(3):
        if not (mask >> k) & 1:
            continue
        v, L, l0 = x[:, k].copy(), float(length[k]), float(lo[k])
        q = np.floor((v - l0) / L)
        v = v - q * L
        add = q.astype(np.int64)
        up = v >= l0 + L
        v[up] = l0
        add[up] += 1
        v[v < l0] = l0
        x[:, k] = v
        image[:, k] += add.astype(np.int32)
    return x, image


def unwrap(x, image, length, mask):
    x = np.asarray(x, dtype=np.float64)
    out = x.copy()
    for k in range(3):
        if (mask >> k) & 1:
            shift = np.asarray(image)[:, k].astype(np.float64) * np.float64(length[k])
            out[:, k] = x[:, k] + shift
    return out


def msd(xu, x0u, mass, members):
    """The ANI_MD_MSD_NOUT outputs of one group (members: bool [n]) from unwrapped positions and origin (fp64, as the kernel forms
    them), the displacement d = xu - x0u in fp64 as the kernel forms it, every sum in np.longdouble, the com-yes part in the direct
    form mean (d_k - dcm_k)^2.  Returns (out [12] float64, terms): terms holds the sums of absolute values, per component, that the
    rounding bound needs: a2 = sum d_k^2, a1 = sum |d_k|, am = sum m |d_k|, and N, M."""
    ld = np.longdouble
    sel = np.asarray(members, dtype=bool)
    out = np.zeros(NOUT)
    N = int(sel.sum())
    if N == 0:
        return out, dict(a2=np.zeros(3), a1=np.zeros(3), am=np.zeros(3), N=0, M=0.0)
    d = (np.asarray(xu, dtype=np.float64) - np.asarray(x0u, dtype=np.float64))[sel]
    m = np.asarray(mass, dtype=np.float64)[sel]
    dl, ml = d.astype(ld), m.astype(ld)[:, None]
    M = ml.sum()
    dcm = (ml * dl).sum(0) / M
    out[0:3] = ((dl * dl).sum(0) / N).astype(np.float64)
    out[3] = float((dl * dl).sum() / N)
    com = ((dl - dcm) ** 2).sum(0) / N
    out[4:7] = com.astype(np.float64)
    out[7] = float(com.sum())
    out[8:11] = dcm.astype(np.float64)
    out[11] = float((~np.isfinite(d).all(1)).sum())
    terms = dict(a2=np.asarray((dl * dl).sum(0), dtype=np.float64), a1=np.asarray(np.abs(dl).sum(0), dtype=np.float64),
                 am=np.asarray((ml * np.abs(dl)).sum(0), dtype=np.float64), N=N, M=float(M))
    return out, terms


def msd_bounds(terms):
    """Absolute bounds on the twelve outputs of a group, from the reference's own terms.

    Every device sum S of terms t_i is formed by roundings in a fixed tree: the term itself (one rounding: d_k^2 or m d_k; d_k
    itself is the reference's own fp64 value), the block sum (6 butterfly levels and 3 additions of the four waves), the strided
    accumulation of the block partials (ceil(nblk / 256) - 1 additions that are not onto a zero, nblk = ceil(N_all / 256)), a
    second block sum (up to 9; 2 where at most four partials exist, the other additions being onto zeros) and one addition less
    than the group has classes.  A term passes through at most `depth` roundings, so |S - sum t_i| <= depth * 2^-53 * sum |t_i| to
    first order.  The bar takes depth = N_g / 256 + 16 with N_g the atoms of the group.  For the sizes of these tests (N_all <=
    66 000, three classes): 1 + 9 + 1 + 9 + 2 = 22 at the largest size, where the smallest group has N_g / 256 > 40; at most
    1 + 9 + 0 + 2 + 2 = 14 below 1 024 atoms; the division by N or M is one more.  The fourth words add two further roundings, which
    at N_g < 256 brings the strict worst case (every rounding a full half ulp in the same direction) to 17 against the bar's 16
    + N_g / 256: there the bar is a hair under the worst case and far above any error that occurs (roundings do not align; the
    tests print both).
        E(S2_k) = depth 2^-53 a2_k     E(S1_k) = depth 2^-53 a1_k     E(Sm_k) = depth 2^-53 am_k
    Outputs:  msd_k = S2_k / N: E(S2_k) / N;  dcm_k = Sm_k / M: E(Sm_k) / M;  the com-yes component
        f = S2 / N - 2 dcm S1 / N + dcm^2:  |df| <= E(S2) / N + 2 |dcm| E(S1) / N + 2 (|S1 / N| + |dcm|) E(dcm) + E(dcm)^2
    (the partial derivatives of the closed form, the last term its second order); the fourth words add their three components'
    bounds.  The count of non-finite atoms is exact."""
    N, M = terms["N"], terms["M"]
    b = np.zeros(NOUT)
    if N == 0:
        return b
    depth = N / 256.0 + 16.0
    e2, e1, em = (depth * EPS * terms[k] for k in ("a2", "a1", "am"))
    edcm = em / M
    dcm_abs, s1_abs = terms["am"] / M, terms["a1"] / N           # |dcm_k| <= am_k / M, |S1_k / N| <= a1_k / N
    b[0:3] = e2 / N
    b[3] = b[0:3].sum()
    b[4:7] = e2 / N + 2.0 * dcm_abs * e1 / N + 2.0 * (s1_abs + dcm_abs) * edcm + edcm ** 2
    b[7] = b[4:7].sum()
    b[8:11] = edcm
    return b


def read_dcd(path):
    """A file of dcd.DCDWriter: dict(nset, first_step, every, last_step, dt, natoms, remarks [2], cell [nf, 3] (the box lengths),
    cosines [nf, 3], xyz [nf, n, 3] float32, size).  Every record's two byte counts are checked."""
    data = open(path, "rb").read()
    at = 0

    def record():
        nonlocal at
        (nb,) = struct.unpack_from("<i", data, at)
        body = data[at + 4: at + 4 + nb]
        (tail,) = struct.unpack_from("<i", data, at + 4 + nb)
        assert tail == nb and len(body) == nb
        at += nb + 8
        return body

    r1 = record()
    assert len(r1) == 84 and r1[:4] == b"CORD"
    ints = struct.unpack_from("<9i", r1, 4)
    (dt,) = struct.unpack_from("<f", r1, 40)
    tail = struct.unpack_from("<10i", r1, 44)
    assert ints[4:] == (0,) * 5 and tail == (1,) + (0,) * 8 + (24,)
    r2 = record()
    assert len(r2) == 164 and struct.unpack_from("<i", r2)[0] == 2
    remarks = [r2[4:84].decode("ascii"), r2[84:164].decode("ascii")]
    r3 = record()
    assert len(r3) == 4
    (natoms,) = struct.unpack("<i", r3)
    assert at == 276
    cells, cosines, frames = [], [], []
    while at < len(data):
        c = np.frombuffer(record(), dtype="<f8")
        assert c.shape == (6,)
        cells.append(c[[0, 2, 5]])
        cosines.append(c[[1, 3, 4]])
        comps = [np.frombuffer(record(), dtype="<f4") for _ in range(3)]
        assert all(a.shape == (natoms,) for a in comps)
        frames.append(np.stack(comps, axis=1))
    return dict(nset=ints[0], first_step=ints[1], every=ints[2], last_step=ints[3], dt=dt, natoms=natoms, remarks=remarks,
                cell=np.array(cells).reshape(-1, 3), cosines=np.array(cosines).reshape(-1, 3),
                xyz=np.array(frames, dtype=np.float32).reshape(-1, natoms, 3), size=len(data))
