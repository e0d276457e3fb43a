"""fp64 references of single stages of the hot path, with error bars derived from the kernels' arithmetic.

The MLP stage (forward through the ensemble + dE/dAEV) is evaluated here in numpy fp64 on the kernel's OWN AEV rows
(``debug_view().d_aev``), so a difference from the kernel comes from the MLP kernels alone.  Units follow the library:
``eatom`` in kcal/mol including the self energy (as ``ANI.compute(...)["eatom"]``), ``gaev`` = the mean over members of
dE/dAEV in Hartree per AEV unit (as ``d_gaev``: the fused kernels scale the backward seed by ``1/M`` and sum members,
``ani_hip_mlp.cpp``, ``G.scale``; the oracle's ``gaev`` has the same scaling).

Error model of the MLP kernels
------------------------------
u = 2^-24 (fp32 unit roundoff).  Every product of a layer, y_o = sum_k w_ok x_k (+ b_o), is bounded componentwise by

    |y_kernel - y_exact| <= rho * S_o + kacc(n) * u * (S_o + |b_o|) + floor_o,     S_o = sum_k |w_ok| |x_k|

* rho, the dropped part of the split arithmetic, per product |w||x|:
  - bf16x3 (mlp_arith 1): both operands are split exactly into three bf16 terms (8 significant bits each); the kernels
    keep six of the nine cross products and drop mid*lo, lo*mid, lo*lo, each at most 2^-8 * 2^-16 of |w||x|:
    rho = 2^-23 = 2u.
  - f16x2 (mlp_arith 2): each operand, scaled by a power of two, is h + l with two fp16 terms good to 2^-22; the
    product of two such operands is good to 2 * 2^-22 + 2^-44 < 9u (rho = 9u).  The low term of a small operand can
    fall below fp16's normal range: it then carries an absolute error of at most half the subnormal spacing, 2^-25, in
    scaled units.  Scales: weights of layer k by ws_k = 2^(13 - e), e the binade of the largest |w| of the layer
    (``ani_hip_model.cpp``, wscale); forward activations by 2^4, backward gradients by 2^12.  So floor_o =
    2^-25 (sum_k |x_k| / ws + sum_k |w_ok| / a_scale).  bf16 has fp32's exponent range: floor = 0.
* kacc(n): the fp32 accumulation of n terms, n = K * (number of split products: 6 or 3), plus the bias and the
  power-of-two rescale (exact).  The worst case is (n - 1) u; we use the probabilistic bound of Higham & Mary
  (SIAM J. Sci. Comput. 41 (2019) A2815): rounding errors of a sum are mean-independent and bounded by u, so the error
  exceeds lambda sqrt(n) u sum|terms| with probability at most 2 exp(-lambda^2 / 2).  lambda = 8 gives 2.5e-14 per
  element, far below one false alarm in a suite's worth of checked elements (~1e8).  kacc(n) = 8 sqrt(n) + 2.  The
  worst case K u would let a single-term bf16 product of the first layer through (its error is ~2^-9 sqrt(K) of the
  row's rms term), which is the slip these bars exist to catch.
* CELU: h = z for z > 0, alpha (exp(z / alpha) - 1) otherwise, 1-Lipschitz: the error of z passes through, plus the
  evaluation of exp (within 2 ulp) and the subtraction: 4 u (|h| + alpha).
* CELU derivative, taken from the stored activation: c = 1 for h > 0, h / alpha + 1 otherwise.  An error E in h becomes
  E / alpha in c, plus 2 u for the multiply-add; where the reference's h exceeds E the kernel sees h > 0 too and
  c = 1 exactly.  This is the one amplification of the stage: 1 / alpha = 10 for CELU(0.1).
* the output layer (1 wide) runs in plain fp32 in the epilogue: rho = 0, kacc(d_L).
* the members are summed in fp32 (energies, and dE/dAEV rows of the (tile, member) items): kacc(M) on sum |member terms|.
* eatom = (e + self energy) * 627.509..., formed in fp64 from an fp32 e: one more u |e|.

The forward errors are carried layer by layer, the backward ones likewise through W^T, first order in u.  They are
carried in quadrature, sqrt(W^2 E_{l-1}^2) + (new error): the error of each component of a layer's output is a sum of
independent rounding errors (the same model as kacc), so through the next product they add like independent variables, and
a bound lambda sigma on each maps to lambda sigma again.  Carried through |W| instead, the bound grows by sum_k |w_k| ~ 25
per layer, which over six products says nothing: a bar a thousand times the kernels' error catches no slip.  The bars are
the carried bounds; each term of them has the form kappa * u * (a magnitude), the magnitudes being sum |w||x| forward and
|W|^T |delta| backward.  Nothing in them was fitted to an observed error.

What these bars cannot see.  They sit 300 to 1000 times above the error the stage makes when it is evaluated in plain fp32
(tests/test_stage_reference_cpu.py measures both), because kacc multiplies sum |terms| while the real rounding error
follows the partial sums, which cancel.  So they catch a product that lost its split (one bf16 term per operand: 5 to 45
times the bar), but NOT a lost low term of the bf16x3 split (hi + mid kept, 16 significant bits): that slip makes 10 to 15
times the fp32 error, 0.01 to 0.07 of the bar, and passes.  It cannot be separated reliably by any bar of this kind: its
error is within a factor lambda = 8 of the rounding noise the bar has to admit with certainty, whatever order the kernel
sums in.  The same holds for eatom, whose bar reaches 0.01 kcal/mol per atom on the 1008-column shapes.  A lost low term
in code all forms share (the operand splits) is therefore not caught by these bars; one lost in a single form shows only
as a difference from the other forms (tests/test_mlp_fused.py), and only where it exceeds that test's tolerances.

The AEV-backward stage has its fp64 reference in the oracle: ``Oracle.aev_vjp`` runs pass C of the oracle on a dE/dAEV the
caller supplies (the kernel's own ``d_gaev``, mapped to centres and full width), and returns beside forces and virial the
sums of the absolute values of their terms, the magnitudes a bar of that stage is written in.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
HARTREE2KCALMOL = 627.5094738898777
LAMBDA = 8.0

# arithmetic -> (planes of the split, rho in units of u, forward activation scale, backward gradient scale, has a floor)
ARITH = {1: dict(products=6, rho=2.0, a_fwd=1.0, a_bwd=1.0, floor=False),
         2: dict(products=3, rho=9.0, a_fwd=16.0, a_bwd=4096.0, floor=True)}


def kacc(n):
    """kappa of an fp32 sum of n terms (probabilistic, see the module docstring)"""
    return LAMBDA * math.sqrt(max(int(n), 1)) + 2.0


def _wscale(Ws):
    """power of two of the fp16 weight planes of one layer (all members), as ani_hip_model.cpp computes it"""
    wmax = max(float(np.abs(W).max()) for W in Ws)
    if wmax == 0:
        return 1.0
    _, e = math.frexp(wmax)
    return 2.0 ** max(-24, min(24, 13 - e))


def full_width_rows(ani, nlocal):
    """The kernel's AEV rows, one per centre (in centre order), mapped back to the model's full AEV width; plus the row
    index of every centre and the debug view."""
    v = ani.debug_view()
    A = v.aev_active_length
    rows = ani.debug_read(v.d_row_of_centre, (nlocal,), np.int32)
    aev = ani.debug_read(v.d_aev, (v.nrows, v.aev_stride), np.float32)
    cm = ani.colmap()
    full = np.zeros((nlocal, ani.aev_length), np.float64)
    full[:, cm] = aev[rows, :A]
    return full, rows, v, cm


def full_width_gaev(ani, nlocal):
    """The kernel's dE/dAEV rows (``d_gaev``), one per centre (in centre order), at the model's full AEV width: rows through
    ``d_row_of_centre``, columns through ``colmap()``.  The columns of absent species, which the kernels do not hold, are zero:
    no neighbour contributes to them, so they carry no force.  This is what ``Oracle.aev_vjp`` takes."""
    v = ani.debug_view()
    A = v.aev_active_length
    rows = ani.debug_read(v.d_row_of_centre, (nlocal,), np.int32)
    g = ani.debug_read(v.d_gaev, (v.nrows, v.aev_stride), np.float32)
    full = np.zeros((nlocal, ani.aev_length), np.float64)
    full[:, ani.colmap()] = g[rows, :A]
    return full


def _celu(z, alpha):
    return np.where(z > 0, z, alpha * np.expm1(np.minimum(z, 0) / alpha))


def mlp_stage(model, x, species, arith=None, dtype=np.float64, mutate=None):
    """The ensemble on AEV rows x [n, aev_len] (full width) of centres of the given species.

    Returns dict(eatom [n] kcal/mol, gaev [n, aev_len] Hartree, and when ``arith`` is 1 or 2 the bars eatom_bar [n] and
    gaev_bar [n, aev_len] of that split arithmetic).  ``dtype``: np.float64 for the reference, np.float32 to run the same
    arithmetic in fp32 (a soundness check of the bars).  ``mutate``: a function applied to every weight matrix and every
    operand of a product before it is multiplied (emulates a kernel slip, e.g. a single bf16 term)."""
    n, A = x.shape
    M, L, alpha = model.num_models, model.num_layers, float(model.celu_alpha)
    scale = 1.0 / M
    op = mutate if mutate is not None else (lambda a: a)
    e_out = np.zeros(n, np.float64)
    g_out = np.zeros((n, A), np.float64)
    want = arith is not None
    if want:
        cfg = ARITH[arith]
        rho = cfg["rho"] * U
        e_bar = np.zeros(n)
        g_bar = np.zeros((n, A))
        e_abs = np.zeros(n)     # sum over members of |member energy|: the fp32 member sum
        g_abs = np.zeros((n, A))
    for s in range(model.num_species):
        idx = np.nonzero(species == s)[0]
        if idx.size == 0:
            continue
        X = x[idx].astype(dtype)
        for a in range(M):
            Ws = [model.weights[a][s][l][0] for l in range(L)]
            bs = [model.weights[a][s][l][1] for l in range(L)]
            ws = [_wscale([model.weights[m][s][l][0] for m in range(M)]) for l in range(L - 1)] if want else None
            # forward
            hs = [X]
            E = [np.zeros_like(X, dtype=np.float64)] if want else None
            for l in range(L):
                W, b, h = Ws[l].astype(dtype), bs[l].astype(dtype), hs[-1]
                if l < L - 1:
                    z = op(h) @ op(W).T + b
                else:
                    z = h @ W.T + b   # the epilogue: plain fp32
                if want:
                    Wa, ha = np.abs(Ws[l].astype(np.float64)), np.abs(h.astype(np.float64))
                    S = ha @ Wa.T
                    K = Wa.shape[1]
                    if l < L - 1:
                        err = np.sqrt(E[-1] ** 2 @ (Wa ** 2).T) + rho * S + kacc(K * cfg["products"] + 1) * U * (S + np.abs(bs[l]))
                        if cfg["floor"]:
                            err = err + 2.0 ** -25 * (ha.sum(1, keepdims=True) / ws[l] + Wa.sum(1)[None, :] / cfg["a_fwd"])
                    else:
                        err = np.sqrt(E[-1] ** 2 @ (Wa ** 2).T) + kacc(K + 1) * U * (S + np.abs(bs[l]))
                if l < L - 1:
                    h = _celu(z, alpha).astype(dtype)
                    if want:
                        err = err + 4 * U * (np.abs(h.astype(np.float64)) + alpha)
                else:
                    h = z
                hs.append(h)
                if want:
                    E.append(err)
            e_out[idx] += scale * hs[-1][:, 0].astype(np.float64)
            # backward: g = dE/dh of layer l's output, seeded with scale at the output
            g = np.broadcast_to(Ws[L - 1].astype(dtype)[0] * dtype(scale), (idx.size, Ws[L - 1].shape[1])).copy()
            if want:
                e_bar[idx] += scale * E[-1][:, 0]
                e_abs[idx] += scale * np.abs(hs[-1][:, 0])
                D = U * np.abs(g.astype(np.float64))   # one fp32 multiply
            for l in range(L - 2, -1, -1):
                hl = hs[l + 1]                       # output of layer l (CELU applied)
                c = np.where(hl > 0, 1.0, hl / alpha + 1.0).astype(dtype)
                delta = g * c
                W = Ws[l].astype(dtype)
                gn = op(delta) @ op(W)
                if want:
                    h64 = hl.astype(np.float64)
                    Eh = E[l + 1]
                    err_c = np.where(h64 > Eh, 0.0, Eh / alpha + 2 * U)
                    g64 = np.abs(g.astype(np.float64))
                    dl = np.abs(delta.astype(np.float64))
                    Wa = np.abs(Ws[l].astype(np.float64))
                    Sb = dl @ Wa
                    K = Wa.shape[0]
                    Dn = np.sqrt(((D * np.abs(c)) ** 2 + (g64 * err_c) ** 2) @ Wa ** 2) + rho * Sb + kacc(K * cfg["products"]) * U * Sb
                    if cfg["floor"]:
                        Dn = Dn + 2.0 ** -25 * (dl.sum(1, keepdims=True) / ws[l] + Wa.sum(0)[None, :] / cfg["a_bwd"])
                    D = Dn
                g = gn
            g_out[idx] += g.astype(np.float64)
            if want:
                g_bar[idx] += D
                g_abs[idx] += np.abs(g.astype(np.float64))
    sae = np.asarray(model.self_energies, np.float64)[species]
    out = dict(eatom=(e_out + sae) * HARTREE2KCALMOL, gaev=g_out)
    if want:
        out["eatom_bar"] = (e_bar + kacc(M) * U * e_abs + U * np.abs(e_out)) * HARTREE2KCALMOL
        out["gaev_bar"] = g_bar + kacc(M) * U * g_abs
    return out


def bf16_single(a):
    """a rounded to one bf16 term (round to nearest even): the product a kernel would form if it lost the split"""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    b = a32.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).astype(a.dtype)


def bf16_hi_mid(a):
    """a as the first two terms of its three-way bf16 split (the low term lost): 16 significant bits"""
    hi = bf16_single(a)
    return (hi + bf16_single(np.asarray(a, np.float32) - hi)).astype(a.dtype)


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar (0 / 0 counts as 0)"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bar)
    return float(np.nanmax(r)) if r.size else 0.0
