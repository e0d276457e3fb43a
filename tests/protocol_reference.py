"""NumPy references for the kernels of include/ani_md_protocol.h, written from the header's text: every expression in the header's
operation order, without fused multiply-adds (NumPy has none), the block sums and the finish in the header's fixed order.

com_sample        ani_md_com_sample: the record, and the sums of magnitudes that the rounding bounds are made of
com_apply         ani_md_com_apply
com_bounds        bounds on the record from those magnitudes
residual_bounds   bounds on the momentum and angular momentum that a sample finds after an apply

The sample and the apply round every operation on its own, and so does this file: the bounds below hold for any order of the
sums, the fixed order is only what makes two calls agree bitwise.
"""
import numpy as np

EPS = 2.0 ** -53
BLOCK = 256
FTM2V = 1.0 / 48.88821291 / 48.88821291
MVV2E = 48.88821291 * 48.88821291
BOLTZ = 0.0019872067

COM_NREC = 24
C_MASS, C_XCM, C_VCM, C_ANGMOM, C_INERTIA, C_OMEGA, C_SINGULAR, C_NONFINITE, C_COUNT = 0, 1, 4, 7, 10, 16, 19, 20, 21


# ---- sums in the kernels' order --------------------------------------------------------------------------------------------
def block_sums(values):
    """[nblk] block sums of values [n] in blocks of 256 (zeros behind the end): xor butterflies 32, 16, .. 1 inside each wave of 64,
    then ((w0 + w1) + w2) + w3"""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    nblk = max((values.size + BLOCK - 1) // BLOCK, 1)
    a = np.zeros(nblk * BLOCK)
    a[: values.size] = values
    a = a.reshape(nblk, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[:, :, lane ^ off]
    w = a[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def finish(partials):
    """the sum of block partials by one workgroup: thread t adds partials t, t + 256, ... in ascending order onto 0, then the block sum"""
    partials = np.asarray(partials, dtype=np.float64).reshape(-1)
    acc = np.zeros(BLOCK)
    for base in range(0, partials.size, BLOCK):
        chunk = partials[base: base + BLOCK]
        acc[: chunk.size] = acc[: chunk.size] + chunk
    return float(block_sums(acc)[0])


def kinetic(m, v):
    return float(0.5 * MVV2E * (np.asarray(m)[:, None] * v * v).sum())


# ---- centre of mass ---------------------------------------------------------------------------------------------------------
def _unwrapped(x, image, length, mask):
    x = np.asarray(x, dtype=np.float64)
    if image is None:
        return x.copy()
    out = x.copy()
    for k in range(3):
        if (mask >> k) & 1:
            out[:, k] = x[:, k] + np.asarray(image)[:, k].astype(np.float64) * np.float64(length[k])
    return out


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def com_sample(x, image, v, mass, ref, length, mask):
    """(record [24], terms): the header's two launches; terms: the sums of magnitudes behind each of the sixteen sums (aM, ad [3],
    ap [3], al [3], asq [6]) and n"""
    x, v, m = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(mass, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    n = x.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        d = _unwrapped(x, image, length, mask) - ref
        md = m[:, None] * d
        cols = [m] + [md[:, k] for k in range(3)] + [m * v[:, k] for k in range(3)]
        cols += [m * (d[:, 1] * v[:, 2] - d[:, 2] * v[:, 1]), m * (d[:, 2] * v[:, 0] - d[:, 0] * v[:, 2]),
                 m * (d[:, 0] * v[:, 1] - d[:, 1] * v[:, 0])]
        cols += [md[:, a] * d[:, b] for a, b in PAIRS]
        cols.append((~(np.isfinite(d).all(1) & np.isfinite(v).all(1))).astype(np.float64))
        S = [finish(block_sums(c)) for c in cols]
        rec = np.zeros(COM_NREC)
        M, P = S[0], np.array(S[4:7])
        c = np.array(S[1:4]) / M
        rec[C_MASS] = M
        rec[C_XCM:C_XCM + 3] = ref + c
        rec[C_VCM:C_VCM + 3] = P / M
        L = np.array(S[7:10]) - _cross(c, P)
        C = {ab: S[10 + j] - M * c[ab[0]] * c[ab[1]] for j, ab in enumerate(PAIRS)}
        Ixx, Iyy, Izz = C[1, 1] + C[2, 2], C[0, 0] + C[2, 2], C[0, 0] + C[1, 1]
        Ixy, Ixz, Iyz = -C[0, 1], -C[0, 2], -C[1, 2]
        rec[C_ANGMOM:C_ANGMOM + 3] = L
        rec[C_INERTIA:C_INERTIA + 6] = [Ixx, Iyy, Izz, Ixy, Ixz, Iyz]
        Axx, Ayy, Azz = Iyy * Izz - Iyz * Iyz, Ixx * Izz - Ixz * Ixz, Ixx * Iyy - Ixy * Ixy
        Axy, Axz, Ayz = Ixz * Iyz - Ixy * Izz, Ixy * Iyz - Ixz * Iyy, Ixy * Ixz - Ixx * Iyz
        det = (Ixx * Axx + Ixy * Axy) + Ixz * Axz
        tr3 = ((Ixx + Iyy) + Izz) / 3.0
        singular = bool(n < 2 or abs(det) <= 1e-12 * ((tr3 * tr3) * tr3))
        if not singular:
            rec[C_OMEGA:C_OMEGA + 3] = [((Axx * L[0] + Axy * L[1]) + Axz * L[2]) / det, ((Axy * L[0] + Ayy * L[1]) + Ayz * L[2]) / det,
                                        ((Axz * L[0] + Ayz * L[1]) + Azz * L[2]) / det]
        rec[C_SINGULAR], rec[C_NONFINITE], rec[C_COUNT] = float(singular), S[16], float(n)
        ad, av = np.abs(d), np.abs(v)
        terms = dict(n=n, aM=float(m.sum()), ad=(m[:, None] * ad).sum(0), ap=(m[:, None] * av).sum(0),
                     al=np.array([(m * (ad[:, 1] * av[:, 2] + ad[:, 2] * av[:, 1])).sum(), (m * (ad[:, 2] * av[:, 0] + ad[:, 0] * av[:, 2])).sum(),
                                  (m * (ad[:, 0] * av[:, 1] + ad[:, 1] * av[:, 0])).sum()]),
                     asq=np.array([(m * ad[:, a] * ad[:, b]).sum() for a, b in PAIRS]))
    return rec, terms


def com_bounds(rec, terms):
    """Absolute bounds on MASS, XCM, VCM, ANGMOM and INERTIA of a record, |device - this reference| and |either - exact|.

    A sum of n terms in the kernels' tree passes each term through at most depth roundings: up to 4 in the term itself (the cross
    product's two products, its difference and the mass), 9 in the block sum, ceil(nblk / 256) in the strided accumulation, 9 in the
    second block sum; depth = n / 256 + 24 is above that for every n (nblk / 256 <= n / 65536 + 1).  So E(S) = depth 2^-53 sum |term|,
    with the sums of magnitudes of com_sample's terms.  Then, to first order, with c = Sd / M:
        E(M) = depth 2^-53 aM          E(c_k) = (E(Sd_k) + |c_k| E(M)) / M + 2^-53 |c_k|      XCM_k: E(c_k) + 2^-53 (|ref_k| + |c_k|)
        VCM_k: (E(P_k) + |VCM_k| E(M)) / M + 2^-53 |VCM_k|
        ANGMOM_x: E(Sl_x) + |c_y| E(P_z) + |P_z| E(c_y) + |c_z| E(P_y) + |P_y| E(c_z) + 4 2^-53 (|Sl_x| + |c_y P_z| + |c_z P_y|), cyclic
        C_ab = S_ab - M c_a c_b: E(S_ab) + |c_a c_b| E(M) + M (|c_a| E(c_b) + |c_b| E(c_a)) + 4 2^-53 (|S_ab| + M |c_a c_b|)
        INERTIA: the diagonal words add the bounds of their two C's and one rounding, the others are a C with its sign changed.
    Magnitudes are taken from the sums of magnitudes (|Sd_k| <= ad_k and so on), so nothing of the result under test enters.
    Returns a dict of arrays: mass, xcm, vcm, angmom, inertia."""
    n, M = terms["n"], terms["aM"]
    depth = n / 256.0 + 24.0
    eM = depth * EPS * M
    ed, ep, el, es = (depth * EPS * terms[k] for k in ("ad", "ap", "al", "asq"))
    c, vcm = terms["ad"] / M, terms["ap"] / M                     # bounds on |c_k| and |VCM_k|
    ec = (ed + c * eM) / M + EPS * c
    ref = np.abs(rec[C_XCM:C_XCM + 3]) + c                        # |ref_k| <= |XCM_k| + |c_k|
    out = dict(mass=np.array([eM]), xcm=ec + EPS * (ref + c), vcm=(ep + vcm * eM) / M + EPS * vcm)
    P = terms["ap"]
    ang = np.zeros(3)
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        ang[k] = el[k] + c[a] * ep[b] + P[b] * ec[a] + c[b] * ep[a] + P[a] * ec[b] + 4.0 * EPS * (terms["al"][k] + c[a] * P[b] + c[b] * P[a])
    out["angmom"] = ang
    eC = np.array([es[j] + c[a] * c[b] * eM + M * (c[a] * ec[b] + c[b] * ec[a]) + 4.0 * EPS * (terms["asq"][j] + M * c[a] * c[b])
                   for j, (a, b) in enumerate(PAIRS)])
    mag = terms["asq"] + M * np.array([c[a] * c[b] for a, b in PAIRS])
    out["inertia"] = np.array([eC[1] + eC[2] + EPS * (mag[1] + mag[2]), eC[0] + eC[2] + EPS * (mag[0] + mag[2]),
                               eC[0] + eC[1] + EPS * (mag[0] + mag[1]), eC[3], eC[4], eC[5]])
    return out


def residual_bounds(before, after, terms_before, terms_after, linear, angular):
    """Bounds on |P| = M |VCM| and |L| = |ANGMOM| of a sample taken AFTER an apply that used the record `before`.

    Linear.  In exact arithmetic sum m (v - VCM) = 0.  What is left: the error of VCM times M (com_bounds of the record before), one
    rounding per subtracted component (2^-53 sum m |v'|), and the error of the second sample (depth 2^-53 sum m |v'|).
    Angular.  In exact arithmetic L' = L - I omega = 0.  What is left: the errors of L and of I omega as the first sample has them
    (bounds of ANGMOM, and of INERTIA times |omega|), the cofactor solve (about 30 roundings of products bounded by |I|^2 |L|, divided
    by det: 32 2^-53 cond(I) |I| |omega| covers it, with |I| the largest |entry| times 3 and cond from the reference's own tensor),
    the roundings of the apply (6 per component: 6 2^-53 sum m |r x (omega x r)| <= 6 2^-53 |omega| sum m |r|^2 ~ tr I |omega|), and the
    second sample's error.  Without the linear part the momentum that stays feeds c x P rounding only, which ANGMOM's bound holds."""
    b0, b1 = com_bounds(before, terms_before), com_bounds(after, terms_after)
    M = terms_before["aM"]
    depth = terms_after["n"] / 256.0 + 24.0
    out = {}
    if linear:
        out["P"] = M * b0["vcm"] + (depth + 1.0) * EPS * terms_after["ap"] + M * b1["vcm"]
    if angular:
        I6 = before[C_INERTIA:C_INERTIA + 6]
        I = np.array([[I6[0], I6[3], I6[4]], [I6[3], I6[1], I6[5]], [I6[4], I6[5], I6[2]]])
        w = np.abs(before[C_OMEGA:C_OMEGA + 3]).max()
        normI = 3.0 * np.abs(I).max()
        cond = np.linalg.cond(I)
        iw = b0["inertia"].max() * 3.0 * w
        out["L"] = b0["angmom"] + iw + 32.0 * EPS * cond * normI * w + 6.0 * EPS * normI * w + b1["angmom"]
    return out


def com_apply(x, v, image, rec, flags, target, dim_mask, length, mask, x_built=None, d2max=0.0):
    """(x, v, d2max) after ani_md_com_apply (new arrays)"""
    x, v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
    if rec[C_NONFINITE] != 0.0:
        return x, v, float(d2max)
    if flags & 1:
        v = v - rec[C_VCM:C_VCM + 3]
    if flags & 2:
        r = _unwrapped(x, image, length, mask) - rec[C_XCM:C_XCM + 3]
        w = np.broadcast_to(rec[C_OMEGA:C_OMEGA + 3], r.shape)
        v = v - _cross(w, r)
    if flags & 4:
        for k in range(3):
            if (dim_mask >> k) & 1:
                x[:, k] = x[:, k] + (target[k] - rec[C_XCM + k])
        if x_built is not None:
            d = x - x_built
            d2 = ((0.0 + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            d2max = max(float(d2max), float(d2.max()))
    return x, v, float(d2max)
