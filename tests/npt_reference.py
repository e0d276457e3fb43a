"""numpy forms of the isotropic Nose-Hoover barostat, written from the contract in include/ani_md.h (ani_md_npt_*): the reference of
every barostat test.  The chain is nh_reference.chain_half_step -- one chain for the thermostat and the barostat, as on the device.

From the header.  N owned atoms; tdof, kt = k_B t_target, K2 = sum m v^2 mvv2e; Wtr = (ev[1] + ev[5]) + ev[9]; V = (len0 len1) len2;
W = ((N + 1) kt) (p_period p_period); wd the one scalar strain rate; c the fixed point (the box centre at the start).
  barostat chain:  chain_half_step(K2 := (W wd) wd, t_target, tdof := 1, dt, t_period := p_period, drag := 0, M := mpchain,
                   nc := nc_pchain), then wd *= s
  strain rate:     P = (K2 + Wtr) / (3 V) nktv2p;  wd += dt/2 (((P - p_target) V / nktv2p + K2 / (3 N)) / W)
  first half:      1 barostat chain  2 thermostat chain on K2 (s; K2 *= s^2)  3 strain rate  4 fv = exp(-dt/2 (wd (1 + 1/N))),
                   mu = exp(dt/2 wd)  5 v = (s fv) v; v += dtfm f; x = c + mu (x - c); x += dt v; x = c + mu (x - c)
                   6 lo = c + mu^2 (lo - c); len *= mu^2; ratio = len_new / len_old; omega += dt wd  7 ghost shifts *= ratio
  second half:     1 v += dtfm f; v *= fv  2 K2  3 strain rate (new K2, new Wtr)  4 thermostat chain, v *= s  5 barostat chain
  conserved:       pe + ke + ecouple(thermostat) + 3 (W wd^2 / 2 + ecouple(barostat chain)) + p_target (V - V0) / nktv2p
  a half-step that finds K2, Wtr or the new wd non-finite: s = fv = mu = ratio = 1, box, wd and chains stay, counted.

`half_step` is ani_md_npt_chain in the precision of `dtype`; `npt_initial_integrate` / `npt_final_integrate` are the per-atom
kernels in the operation order of tests/md_loop_reference.py, without fused multiply-adds; `npt_trajectory` is the barostatted
velocity Verlet with a force callback; `rebuild_limit` mirrors lammps_ani_amd.md.npt_rebuild_limit for its derivation's test.

Bars of the device test of ani_md_npt_chain (`half_step_bars`): per output, ten times the difference between `half_step` in
float64 and in np.longdouble on that case, floored: the two chains' outputs at nh_reference.chain_bars (the barostat chain's case
being K2 = W wd^2, tdof 1, p_period), every other output at 1e-14 of the sum of the magnitudes of the terms it is made of (1e-13 for
wd, as chain_bars has it for eta_dot: wd passes through the chain's exponentials).
"""
import functools
import math

import numpy as np

import md_loop_reference as mr
import nh_reference as nh
from nh_reference import BOLTZ, FTM2V, MVV2E, NKTV2P

NSTATE = 56
(PS_COUNT, PS_WD, PS_OMEGA, PS_P, PS_PTARGET, PS_W, PS_FV, PS_MU, PS_LO, PS_LEN, PS_RATIO, PS_C, PS_V0, PS_ECOUPLE, PS_NONFINITE,
 PS_NATOMS, PS_ETA, PS_ETADOT, PS_ETADOTDOT, PS_ECHAIN, PS_VOL) = (0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 14, 17, 20, 21, 22, 23, 24, 32, 40,
                                                                   48, 49)


# ---- the record --------------------------------------------------------------------------------------------------------------
def init_record(lo, length, n):
    """ani_md_npt_init"""
    rec = np.zeros(NSTATE)
    lo, length = np.asarray(lo, dtype=np.float64), np.asarray(length, dtype=np.float64)
    rec[PS_LO:PS_LO + 3], rec[PS_LEN:PS_LEN + 3], rec[PS_RATIO:PS_RATIO + 3] = lo, length, 1.0
    rec[PS_C:PS_C + 3] = lo + 0.5 * length
    rec[PS_FV] = rec[PS_MU] = 1.0
    rec[PS_V0] = rec[PS_VOL] = (length[0] * length[1]) * length[2]
    rec[PS_NATOMS] = n
    return rec


def volume(rec):
    return float((rec[PS_LEN] * rec[PS_LEN + 1]) * rec[PS_LEN + 2])


# ---- ani_md_npt_chain --------------------------------------------------------------------------------------------------------
def half_step(phase, ns, ps, K2, wtr, t_target, p_target, tdof, dt, t_period, drag, p_period, M, nc, Mp, ncp, dtype=np.float64):
    """One call of ani_md_npt_chain.  ns: the NH record (nh_reference.NSTATE doubles), ps: the barostat record; K2: the sum it
    starts from; wtr: the virial's trace.  Returns (ns_new, ps_new, info): new records in `dtype` (the inputs are not written), info
    with the magnitudes the bars are floored by and the two chains' dicts."""
    f = dtype
    ns_in, ps_in = np.asarray(ns, dtype=np.float64), np.asarray(ps, dtype=np.float64)
    ns, ps = ns_in.astype(dtype), ps_in.astype(dtype)
    K2_in, wtr, dt, pt = f(K2), f(wtr), f(dt), f(p_target)
    K2 = K2_in
    N = ps[PS_NATOMS]
    kt = f(BOLTZ) * f(t_target)
    pp = f(p_period)
    W = ((N + f(1.0)) * kt) * (pp * pp)
    lo, ln, c = ps[PS_LO:PS_LO + 3].copy(), ps[PS_LEN:PS_LEN + 3].copy(), ps[PS_C:PS_C + 3].copy()
    V = (ln[0] * ln[1]) * ln[2]
    wd = ps[PS_WD]
    hdt = f(0.5) * dt
    th = dict(eta=ns[8:8 + M], eta_dot=ns[16:16 + M], eta_dotdot=ns[24:24 + M])
    ba = dict(eta=ps[PS_ETA:PS_ETA + Mp], eta_dot=ps[PS_ETADOT:PS_ETADOT + Mp], eta_dotdot=ps[PS_ETADOTDOT:PS_ETADOTDOT + Mp])
    info = {}

    def baro_chain(wd):
        Kb = (W * wd) * wd
        r = nh.chain_half_step(Kb, t_target, 1.0, dt, p_period, 0.0, Mp, ncp, ba["eta"], ba["eta_dot"], ba["eta_dotdot"], dtype)
        info["baro"], info["baro_K2_in"], info["baro_in"] = r, float(Kb), {k: np.asarray(v, dtype=np.float64) for k, v in ba.items()}
        return wd * r["s"], r

    def thermo_chain(K2):
        r = nh.chain_half_step(K2, t_target, tdof, dt, t_period, drag, M, nc, th["eta"], th["eta_dot"], th["eta_dotdot"], dtype)
        info["thermo"], info["thermo_K2_in"] = r, float(K2)
        return r["K2"], r

    def strain(wd, K2):
        P = (K2 + wtr) / (f(3.0) * V) * f(NKTV2P)
        a, b = (P - pt) * V / f(NKTV2P), K2 / (f(3.0) * N)
        info["wd_mag"] = float(abs(wd) + hdt * ((K2 + abs(wtr)) / f(3.0) + abs(pt) * V / f(NKTV2P) + abs(b)) / W)
        info["P_mag"] = float((abs(K2) + abs(wtr)) / (f(3.0) * V) * f(NKTV2P))
        return wd + hdt * ((a + b) / W), P

    with np.errstate(all="ignore"):
        if phase == 0:
            wd, rb = baro_chain(wd)
            K2, rt = thermo_chain(K2)
            wd, P = strain(wd, K2)
        else:
            wd, P = strain(wd, K2)
            K2, rt = thermo_chain(K2)
            wd, rb = baro_chain(wd)
    ns[3], ns[5], ns[7], ps[PS_PTARGET] = f(t_target), f(tdof), f(0.0), pt
    if not (np.isfinite(K2_in) and np.isfinite(wtr) and np.isfinite(wd)):
        ns[1], ns[2], ns[6] = K2_in, f(1.0), ns[6] + f(1.0)
        ps[PS_FV] = ps[PS_MU] = f(1.0)
        ps[PS_RATIO:PS_RATIO + 3] = f(1.0)
        ps[PS_NONFINITE] += f(1.0)
        return ns, ps, info
    Vnew = V
    if phase == 0:
        fv, mu = np.exp(-hdt * (wd * (f(1.0) + f(1.0) / N))), np.exp(hdt * wd)
        mu2 = mu * mu
        lnew = ln * mu2
        ps[PS_FV], ps[PS_MU] = fv, mu
        ps[PS_LO:PS_LO + 3] = c + mu2 * (lo - c)
        ps[PS_LEN:PS_LEN + 3] = lnew
        ps[PS_RATIO:PS_RATIO + 3] = lnew / ln
        Vnew = (lnew[0] * lnew[1]) * lnew[2]
        ps[PS_OMEGA] = ps[PS_OMEGA] + dt * wd
    ns[0], ns[1], ns[2], ns[4] = ns[0] + f(1.0), rt["K2"], rt["s"], rt["ecouple"]
    ns[8:8 + M], ns[16:16 + M], ns[24:24 + M] = rt["eta"], rt["eta_dot"], rt["eta_dotdot"]
    ps[PS_COUNT] += f(1.0)
    ps[PS_WD], ps[PS_P], ps[PS_W], ps[PS_VOL], ps[PS_ECHAIN] = wd, P, W, Vnew, rb["ecouple"]
    ps[PS_ETA:PS_ETA + Mp], ps[PS_ETADOT:PS_ETADOT + Mp], ps[PS_ETADOTDOT:PS_ETADOTDOT + Mp] = rb["eta"], rb["eta_dot"], rb["eta_dotdot"]
    terms = [f(3.0) * (f(0.5) * W * wd * wd), f(3.0) * rb["ecouple"], pt * (Vnew - ps[PS_V0]) / f(NKTV2P)]
    ps[PS_ECOUPLE] = f(3.0) * (f(0.5) * W * wd * wd + rb["ecouple"]) + pt * (Vnew - ps[PS_V0]) / f(NKTV2P)
    info["ecouple_mag"] = float(abs(terms[0]) + f(3.0) * rb["ecouple_mag"] + abs(pt) * (Vnew + ps[PS_V0]) / f(NKTV2P))
    info["box_mag"] = np.asarray(np.abs(c) + np.abs(lo - c) + ln, dtype=np.float64)
    return ns, ps, info


def draw_npt_case(rng):
    """nh_reference.draw_chain_case extended by the barostat's inputs: N in [30, 1e5] (log-uniform; tdof = 3 N - 3), a box of 8 to
    40 A^3 per atom with sides within 25 % of a cube, lo in [-10, 10], c within the middle fifth of the box, V0 within 10 % of V,
    Wtr = +-[0.01, 3] K2 (log-uniform), p_target in [0, 2000] atm, p_period in [100, 2000] fs, |wd| in [1e-7, 1e-4] / fs
    (log-uniform, either sign), mpchain in 1..8, nc_pchain in 1..3, barostat chain: |eta| <= 2, |eta_dot| in [1e-5, 1e-3] / fs,
    |eta_dotdot| <= 1 / p_period^2; omega in [-0.1, 0.1]."""
    def logu(lo, hi, size=None):
        return np.exp(rng.uniform(np.log(lo), np.log(hi), size))

    def sign(size=None):
        return np.where(rng.random(size) < 0.5, -1.0, 1.0)

    c = nh.draw_chain_case(rng)
    N = float(np.round(logu(30.0, 1.0e5)))
    ket_old = c["tdof"] * BOLTZ * c["t_target"]
    c["tdof"] = 3.0 * N - 3.0
    c["K2"] = c["K2"] / ket_old * (c["tdof"] * BOLTZ * c["t_target"])
    V = N * rng.uniform(8.0, 40.0)
    sides = rng.uniform(0.8, 1.25, 3)
    length = sides * (V / sides.prod()) ** (1.0 / 3.0)
    lo = rng.uniform(-10.0, 10.0, 3)
    Mp = int(rng.integers(1, 9))
    p_period = float(rng.uniform(100.0, 2000.0))
    ps = np.zeros(NSTATE)
    ps[PS_COUNT], ps[PS_WD], ps[PS_OMEGA] = 6.0, float(sign() * logu(1e-7, 1e-4)), float(rng.uniform(-0.1, 0.1))
    ps[PS_P], ps[PS_PTARGET], ps[PS_W], ps[PS_FV], ps[PS_MU] = -1.0, -2.0, -3.0, -4.0, -5.0
    ps[PS_LO:PS_LO + 3], ps[PS_LEN:PS_LEN + 3], ps[PS_RATIO:PS_RATIO + 3] = lo, length, -6.0
    ps[PS_C:PS_C + 3] = lo + length * rng.uniform(0.4, 0.6, 3)
    ps[PS_V0] = float(length.prod() * rng.uniform(0.9, 1.1))
    ps[PS_ECOUPLE], ps[PS_NONFINITE], ps[PS_NATOMS], ps[PS_ECHAIN], ps[PS_VOL] = -7.0, 1.0, N, -8.0, -9.0
    ps[PS_ETA:PS_ETA + Mp] = rng.uniform(-2.0, 2.0, Mp)
    ps[PS_ETADOT:PS_ETADOT + Mp] = sign(Mp) * logu(1e-5, 1e-3, Mp)
    ps[PS_ETADOTDOT:PS_ETADOTDOT + Mp] = rng.uniform(-1.0, 1.0, Mp) / p_period ** 2
    c.update(N=N, Mp=Mp, ncp=int(rng.integers(1, 4)), p_period=p_period, p_target=float(rng.uniform(0.0, 2000.0)),
             wtr=float(sign() * logu(0.01, 3.0) * c["K2"]), ps=ps,
             ns=nh.state_record(7, c["K2"], -2.0, -3.0, -4.0, -5.0, 2, c["eta"], c["eta_dot"], c["eta_dotdot"]))
    return c


NPT_CASES, NPT_SEED = 256, 2025


@functools.lru_cache(maxsize=None)
def npt_cases():
    rng = np.random.default_rng(NPT_SEED)
    return tuple(draw_npt_case(rng) for _ in range(NPT_CASES))


def case_half_step(phase, c, dtype=np.float64):
    return half_step(phase, c["ns"], c["ps"], c["K2"], c["wtr"], c["t_target"], c["p_target"], c["tdof"], c["dt"], c["t_period"],
                     c["drag"], c["p_period"], c["M"], c["nc"], c["Mp"], c["ncp"], dtype)


def half_step_bars(phase, c):
    """(ns64, ps64, bar_ns [32], bar_ps [56]) of a drawn case: absolute bars per record entry, the recipe of the module docstring;
    entries that are written exactly (counts, targets, N, c, V0) have bar 0."""
    ns, ps, info = case_half_step(phase, c, np.float64)
    nl, pl, _ = case_half_step(phase, c, np.longdouble)
    bn = 10.0 * np.abs(ns - nl).astype(np.float64)
    bp = 10.0 * np.abs(ps - pl).astype(np.float64)
    M, Mp = c["M"], c["Mp"]
    fn, fp = np.zeros(nh.NSTATE), np.zeros(NSTATE)
    tcase = dict(c, K2=info["thermo_K2_in"])
    tb = nh.chain_bars(tcase, info["thermo"])
    fn[1], fn[2], fn[4] = tb["K2"], tb["s"], tb["ecouple"]
    fn[8:8 + M], fn[16:16 + M], fn[24:24 + M] = tb["eta"], tb["eta_dot"], tb["eta_dotdot"]
    bcase = dict(M=Mp, K2=info["baro_K2_in"], dt=c["dt"], eta_dot=info["baro_in"]["eta_dot"], eta_dotdot=info["baro_in"]["eta_dotdot"])
    bb = nh.chain_bars(bcase, info["baro"])
    # the barostat chain's first acceleration is (W wd^2 - kt) / Q[0] with wd an output of the strain-rate update in phase 1: the
    # error of wd enters it twice
    wd_bar = 1e-13 * info["wd_mag"]
    Q0 = float(info["baro"]["Q"][0])
    bb["eta_dotdot"][0] += 2.0 * float(ps[PS_W]) * abs(float(ps[PS_WD])) * wd_bar / Q0 if phase == 1 else 0.0
    fp[PS_ETA:PS_ETA + Mp], fp[PS_ETADOT:PS_ETADOT + Mp], fp[PS_ETADOTDOT:PS_ETADOTDOT + Mp] = bb["eta"], bb["eta_dot"], bb["eta_dotdot"]
    fp[PS_ECHAIN] = bb["ecouple"]
    fp[PS_WD], fp[PS_P], fp[PS_W] = wd_bar, 1e-14 * info["P_mag"], 1e-14 * float(ps[PS_W])
    fp[PS_ECOUPLE] = 1e-14 * info["ecouple_mag"] + 3.0 * float(ps[PS_W]) * abs(float(ps[PS_WD])) * wd_bar
    fp[PS_VOL] = 1e-14 * float(ps[PS_VOL])
    if phase == 0:
        fp[PS_FV] = fp[PS_MU] = 1e-14
        fp[PS_RATIO:PS_RATIO + 3] = 1e-14
        fp[PS_LO:PS_LO + 3] = fp[PS_LEN:PS_LEN + 3] = 1e-14 * info["box_mag"]
        fp[PS_OMEGA] = 1e-14 * (abs(float(c["ps"][PS_OMEGA])) + c["dt"] * info["wd_mag"]) + c["dt"] * wd_bar
    return ns, ps, np.maximum(bn, fn), np.maximum(bp, fp)


# ---- the per-atom kernels (operation order of md_loop_reference, no fused multiply-adds) --------------------------------------
def npt_initial_integrate(x, v, f, dtfm, dt, x_built, d2max, s, fv, mu, c):
    """v = (s fv) v;  v += dtfm f;  x = c + mu (x - c);  x += dt v;  x = c + mu (x - c);  returns (x, v, d2max)"""
    c = np.asarray(c, dtype=np.float64)[None, :]
    v = (s * fv) * v + dtfm[:, None] * f
    x = c + mu * (x - c)
    x = x + dt * v
    x = c + mu * (x - c)
    return x, v, mr._fold(d2max, mr._d2(x, x_built))


def npt_final_integrate(v, f, dtfm, mass, fv):
    """v += dtfm f;  v *= fv;  returns (v, K2 of the new v by fsum)"""
    v = (v + dtfm[:, None] * f) * fv
    return v, nh.k2_sum(v, mass)


def scale_shifts(shift, ratio):
    return shift * np.asarray(ratio, dtype=np.float64)[None, :]


# ---- the re-neighbouring limit with a moving box -------------------------------------------------------------------------------
def rebuild_limit(skin, lo_built, len_built, lo_now, len_now, nimg_max):
    """The squared displacement above which the list is rebuilt: max(0, (skin - nimg_max (d_lo + d_hi)) / 2)^2 with d_lo, d_hi the
    Euclidean displacements of the two box corners since the build.  A pair's distance changes by at most the two owners'
    displacements (against the unscaled x_built: the dilation is in them) plus the change of the image shift between them, at most
    nimg_max |d len| <= nimg_max (d_lo + d_hi).  One image: Neighbor::check_distance with boxcheck."""
    lo_b, len_b, lo_n, len_n = (np.asarray(a, dtype=np.float64) for a in (lo_built, len_built, lo_now, len_now))
    d_lo = float(np.sqrt(((lo_n - lo_b) ** 2).sum()))
    d_hi = float(np.sqrt(((lo_n + len_n - lo_b - len_b) ** 2).sum()))
    return max(0.0, 0.5 * (skin - nimg_max * (d_lo + d_hi))) ** 2


# ---- the trajectory ----------------------------------------------------------------------------------------------------------
def npt_trajectory(x0, v0, mass, evaluate, steps, dt, lo, length, t_start, t_stop=None, t_period=None, p_start=1.0, p_stop=None,
                   p_period=None, M=3, Mp=3, nc=1, ncp=1, drag=0.0, tdof=None, fresh_k2_every_step=True):
    """Barostatted velocity Verlet in the order of VerletRun with set_npt.  evaluate(x, lo, len) -> (forces [n, 3], potential energy,
    virial: its trace, or the 3 x 3 / 9 entries).  Both chains start at rest, wd = 0.  fresh_k2_every_step: every step takes K2 from
    the velocities (step() N times); False: only the first (run(N)).  Returns the records of step 0 .. steps: dicts of x, v, f, pe,
    ke, wtr, lo, len, vol, press, ecouple (both parts), econserve, t_target, p_target, chain (NH record) and baro (barostat record)."""
    mass = np.asarray(mass, dtype=np.float64)
    n = len(mass)
    t_stop = t_start if t_stop is None else t_stop
    p_stop = p_start if p_stop is None else p_stop
    t_period = 100.0 * dt if t_period is None else t_period
    p_period = 1000.0 * dt if p_period is None else p_period
    tdof = 3.0 * n - 3.0 if tdof is None else float(tdof)
    dtfm = (0.5 * dt * FTM2V) / mass
    x, v = np.array(x0, dtype=np.float64), np.array(v0, dtype=np.float64)
    ns, ps = np.zeros(nh.NSTATE), init_record(lo, length, n)

    def trace(w):
        w = np.asarray(w, dtype=np.float64)
        return float(w) if w.ndim == 0 else float((w.reshape(-1)[0] + w.reshape(-1)[4]) + w.reshape(-1)[8])

    def forces():
        f, pe, w = evaluate(x, ps[PS_LO:PS_LO + 3].copy(), ps[PS_LEN:PS_LEN + 3].copy())
        return f, float(pe), trace(w)

    f, pe, wtr = forces()
    t, p = t_start, p_start

    def record():
        k2 = nh.k2_sum(v, mass)
        vol = volume(ps)
        ec = float(ns[4]) + float(ps[PS_ECOUPLE])
        return dict(x=x.copy(), v=v.copy(), f=f.copy(), pe=pe, ke=0.5 * k2, wtr=wtr, lo=ps[PS_LO:PS_LO + 3].copy(),
                    len=ps[PS_LEN:PS_LEN + 3].copy(), vol=vol, press=(k2 + wtr) / (3.0 * vol) * NKTV2P, ecouple=ec,
                    econserve=pe + 0.5 * k2 + ec, t_target=t, p_target=p, chain=ns.copy(), baro=ps.copy())

    out = [record()]
    K2 = nh.k2_sum(v, mass)
    for k in range(1, steps + 1):
        t, p = nh.ramp_target(k, steps, t_start, t_stop), nh.ramp_target(k, steps, p_start, p_stop)
        if fresh_k2_every_step or k == 1:
            K2 = nh.k2_sum(v, mass)
        else:
            K2 = float(ns[1])
        ns, ps, _ = half_step(0, ns, ps, K2, wtr, t, p, tdof, dt, t_period, drag, p_period, M, nc, Mp, ncp)
        x, v, _ = npt_initial_integrate(x, v, f, dtfm, dt, x, 0.0, float(ns[2]), float(ps[PS_FV]), float(ps[PS_MU]), ps[PS_C:PS_C + 3])
        f, pe, wtr = forces()
        v, K2 = npt_final_integrate(v, f, dtfm, mass, float(ps[PS_FV]))
        ns, ps, _ = half_step(1, ns, ps, K2, wtr, t, p, tdof, dt, t_period, drag, p_period, M, nc, Mp, ncp)
        v = nh.scale(v, float(ns[2]))
        out.append(record())
    return out


# ---- calculators -------------------------------------------------------------------------------------------------------------
def smooth_pair_system(n=32, L=10.0, seed=1, T=300.0, mass=16.0):
    """A small analytic periodic system for the conservation test: n atoms on a jittered 4 x 4 x 4 lattice in a cube of side L,
    u(r) = A (1 - r^2 / rc^2)^3 below rc (A = 2 kcal/mol, rc = 4.5 A), minimum image.  Returns (x, v, masses, lo, len, evaluate)."""
    A, RC = 2.0, 4.5
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n] * (L / 4.0) + 0.3 * rng.normal(size=(n, 3))
    m = np.full(n, mass)
    v = rng.normal(size=(n, 3)) * np.sqrt(BOLTZ * T / (m[:, None] * MVV2E))
    v -= v.mean(0)

    def evaluate(x, lo, length):
        d = x[:, None, :] - x[None, :, :]
        d -= length * np.round(d / length)
        r2 = (d * d).sum(-1)
        np.fill_diagonal(r2, 1e9)
        q = np.clip(1.0 - r2 / RC ** 2, 0.0, None)
        pe = 0.5 * A * (q ** 3).sum()
        gg = 3.0 * A * q * q / RC ** 2 * 2.0
        f = (gg[:, :, None] * d).sum(1)
        return f, pe, 0.5 * (gg * r2 * (q > 0)).sum()

    return g, v, m, np.zeros(3), np.full(3, L), evaluate


def oracle_evaluator(model_path, sysm):
    """evaluate(x, lo, len) -> (forces [n, 3] in global order, potential energy, virial [3, 3]) by the CPU oracle on the periodic
    box [lo, lo + len) with the atoms of sysm"""
    import copy
    from lammps_ani_amd import harness as hx
    from oracle import Oracle
    o, n = Oracle(model_path), sysm.natoms

    def evaluate(xx, lo, length):
        s = copy.copy(sysm)
        s.boxlo, s.boxhi = np.array(lo, dtype=np.float64), np.array(lo, dtype=np.float64) + np.array(length, dtype=np.float64)
        xw = s.boxlo + np.mod(xx - s.boxlo, length)
        inp = hx.decompose(s, x_override=xw)
        r = o.compute(inp)
        f = np.zeros((n, 3))
        np.add.at(f, inp.tag[: inp.nlocal], r["force"][: inp.nlocal])
        np.add.at(f, inp.tag[inp.nlocal:], r["force"][inp.nlocal:])
        return f, float(r["energy"]), r["virial"]

    return evaluate


P_PERIOD, P_START = 25.0, 20000.0     # of the water-box tests: chosen on the CPU so that the volume moves (tests/test_npt_md.py)
