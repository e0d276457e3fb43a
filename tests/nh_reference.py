"""numpy forms of the Nose-Hoover chain and the thermo record, written from the contract in include/ani_md.h (ani_md_nh_*,
ani_md_thermo): the reference of every thermostat test.

`chain_half_step` is the chain's half-step in the precision of `dtype` (np.float64, or np.longdouble for the reference's own
rounding); `k2_sum` / `tensor_sums` are the kinetic sums by `math.fsum` (correctly rounded, whatever the order);  `scale`,
`nh_initial_integrate` and `nh_final_integrate` are the scaled integrators in the operation order of tests/md_loop_reference.py,
without fused multiply-adds; `thermo` is the record of ani_md_thermo; `nvt_trajectory` is a thermostatted velocity Verlet that
takes a force callback.  `draw_chain_case` is the input recipe of the chain tests, defined here once.
"""
import functools
import math

import numpy as np

import md_loop_reference as mr

FTM2V = 1.0 / 48.88821291 / 48.88821291   # LAMMPS units real, as lammps_ani_amd.md
MVV2E = 48.88821291 * 48.88821291
BOLTZ = 0.0019872067
NKTV2P = 68568.415
MV2D = 1.0 / 0.602214129
MASSES = np.array([1.008, 12.011, 14.007, 15.999, 32.06, 18.998, 35.45])
NSTATE, MAXCHAIN, THERMO_N = 32, 8, 16
TENSOR = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # xx yy zz xy xz yz
W_INDEX = tuple(1 + 3 * a + b for a, b in TENSOR)


# ---- the chain ---------------------------------------------------------------------------------------------------------------
def chain_masses(t_target, tdof, t_period, M, dtype=np.float64):
    """(kt, ket, Q [M]): Q[0] = ket / tf^2, Q[k >= 1] = kt / tf^2, tf = 1 / t_period"""
    f = dtype
    kt = f(BOLTZ) * f(t_target)
    ket = f(tdof) * kt
    tf = f(1.0) / f(t_period)
    Q = np.array([(ket if k == 0 else kt) / (tf * tf) for k in range(M)], dtype=dtype)
    return kt, ket, Q


def chain_half_step(K2, t_target, tdof, dt, t_period, drag, M, nc, eta, eta_dot, eta_dotdot, dtype=np.float64):
    """One half-step from K2 and the chain's state (arrays of at least M; not written).  Returns a dict: s, K2 (after the scaling),
    eta, eta_dot, eta_dotdot (length M), ecouple, ecouple_mag (the sum of the magnitudes of ecouple's terms), and kt, ket, Q."""
    f = dtype
    K2, dt = f(K2), f(dt)
    kt, ket, Q = chain_masses(t_target, tdof, t_period, M, dtype)
    eta = np.array(eta[:M], dtype=dtype)
    ed = np.concatenate([np.array(eta_dot[:M], dtype=dtype), np.zeros(1, dtype=dtype)])     # eta_dot[M] = 0
    edd = np.array(eta_dotdot[:M], dtype=dtype)
    nf = f(1.0) / f(nc)
    dfac = f(1.0) - dt * f(drag) / f(nc)
    h2, h4, h8 = nf * dt / f(2.0), nf * dt / f(4.0), nf * dt / f(8.0)
    edd[0] = (K2 - ket) / Q[0]
    s = f(1.0)
    for _ in range(nc):
        for k in range(M - 1, 0, -1):
            e = np.exp(-h8 * ed[k + 1])
            ed[k] = ((ed[k] * e + edd[k] * h4) * dfac) * e
        e0 = np.exp(-h8 * ed[1])
        ed[0] = ((ed[0] * e0 + edd[0] * h4) * dfac) * e0
        fac = np.exp(-h2 * ed[0])
        s = s * fac
        K2 = K2 * (fac * fac)
        edd[0] = (K2 - ket) / Q[0]
        for k in range(M):
            eta[k] = eta[k] + h2 * ed[k]
        ed[0] = (ed[0] * e0 + edd[0] * h4) * e0
        for k in range(1, M):
            e = np.exp(-h8 * ed[k + 1])
            ed[k] = ed[k] * e
            edd[k] = (Q[k - 1] * ed[k - 1] * ed[k - 1] - kt) / Q[k]
            ed[k] = (ed[k] + edd[k] * h4) * e
    terms = [ket * eta[0], f(0.5) * Q[0] * ed[0] * ed[0]]
    for k in range(1, M):
        terms += [kt * eta[k], f(0.5) * Q[k] * ed[k] * ed[k]]
    # up to sixteen terms of either sign: summed without a rounding of its own in float64 (fsum), so that the reference's error
    # is that of its terms; the wider type adds them as they come
    ec = f(math.fsum(terms)) if dtype is np.float64 else sum(terms[1:], terms[0])
    return dict(s=s, K2=K2, eta=eta, eta_dot=ed[:M].copy(), eta_dotdot=edd, ecouple=ec, ecouple_mag=sum(abs(t) for t in terms),
                kt=kt, ket=ket, Q=Q)


def state_record(count, K2, s, t_target, ecouple, tdof, nonfinite, eta, eta_dot, eta_dotdot):
    """the ANI_MD_NH_NSTATE doubles of the device record"""
    rec = np.zeros(NSTATE)
    rec[:7] = (count, K2, s, t_target, ecouple, tdof, nonfinite)
    for k, a in enumerate((eta, eta_dot, eta_dotdot)):
        rec[8 + 8 * k: 8 + 8 * k + len(a)] = np.asarray(a, dtype=np.float64)
    return rec


def draw_chain_case(rng):
    """One drawn input of the chain tests: tdof in [30, 3e5] (log-uniform), T in [50, 1000] K, t_period in [20, 200] fs, dt in
    {0.25, 0.5, 1}, M in 1..8, nc in 1..3, |K2 / ket - 1| in [0.01, 1] (log-uniform, either sign), |eta_dot| in [1e-4, 1e-2] / fs
    (log-uniform, either sign), |eta_dotdot| <= 1 / t_period^2, drag 0 or 0.2; |eta| <= 2: eta is the time integral of eta_dot, at most 1e-2 / fs over a
    period of at most 200 fs."""
    def logu(lo, hi, size=None):
        return np.exp(rng.uniform(np.log(lo), np.log(hi), size))

    def sign(size=None):
        return np.where(rng.random(size) < 0.5, -1.0, 1.0)

    tdof = float(np.round(logu(30.0, 3.0e5)))
    T, t_period = float(rng.uniform(50.0, 1000.0)), float(rng.uniform(20.0, 200.0))
    dt, M, nc = float(rng.choice([0.25, 0.5, 1.0])), int(rng.integers(1, 9)), int(rng.integers(1, 4))
    ket = tdof * BOLTZ * T
    K2 = float(ket * (1.0 + sign() * logu(0.01, 1.0)))
    if K2 <= 0.0:
        K2 = float(ket * 1e-3)
    return dict(tdof=tdof, t_target=T, t_period=t_period, dt=dt, M=M, nc=nc, drag=float(rng.choice([0.0, 0.2])), K2=K2,
                eta=rng.uniform(-2.0, 2.0, M), eta_dot=sign(M) * logu(1e-4, 1e-2, M),
                eta_dotdot=rng.uniform(-1.0, 1.0, M) / t_period ** 2)


CHAIN_CASES, CHAIN_SEED = 256, 2024


@functools.lru_cache(maxsize=None)
def chain_cases():
    """the drawn inputs of the chain tests, the same on the CPU (the reference against np.longdouble) and on the device: 256 cases,
    one launch and one read each on the device, which keeps that test at a second or two"""
    rng = np.random.default_rng(CHAIN_SEED)
    return tuple(draw_chain_case(rng) for _ in range(CHAIN_CASES))


def chain_bars(case, ref):
    """The bars of the device test (ten times the reference's own rounding) for the outputs of one half-step: dict of absolute
    bars for eta [M], eta_dot (scalar), eta_dotdot [M], s, K2, ecouple.  ref: chain_half_step of the case.  eta_dotdot[k] is held
    against the magnitudes of its own numerator's terms, from the reference's outputs; eta_dot against the largest input
    |eta_dot| plus dt times the largest |eta_dotdot| that enters it: the accelerations that came in (with the first
    eta_dotdot[0] = (K2 - ket) / Q[0]) serve the first loop, those that go out the second."""
    M, Q, kt, ket = case["M"], ref["Q"], ref["kt"], ref["ket"]
    ed, edd = np.asarray(ref["eta_dot"], dtype=np.float64), np.asarray(ref["eta_dotdot"], dtype=np.float64)
    edd_in = np.asarray(case["eta_dotdot"], dtype=np.float64).copy()
    edd_in[0] = (case["K2"] - ket) / Q[0]
    bar_edd = np.empty(M)
    bar_edd[0] = 5e-13 * float((float(ref["K2"]) + ket) / Q[0])
    for k in range(1, M):
        bar_edd[k] = 5e-13 * float((Q[k - 1] * ed[k - 1] ** 2 + kt) / Q[k])
    return dict(eta=1e-14 * np.maximum(1.0, np.abs(np.asarray(ref["eta"], dtype=np.float64))),
                eta_dot=1e-13 * float(np.abs(case["eta_dot"]).max() + case["dt"] * max(np.abs(edd_in).max(), np.abs(edd).max())),
                eta_dotdot=bar_edd, s=1e-14 * float(ref["s"]), K2=1e-14 * float(ref["K2"]), ecouple=1e-14 * float(ref["ecouple_mag"]))


# ---- the sums ----------------------------------------------------------------------------------------------------------------
def k2_sum(v, mass):
    """sum_i m_i |v_i|^2 mvv2e: the terms in double precision (a few roundings each, all terms positive), their sum by fsum"""
    m = np.asarray(mass, dtype=np.float64)
    return math.fsum(((m * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])) * MVV2E).tolist())


def tensor_sums(v, mass):
    """[6] sums K_ab = sum_i m_i v_ia v_ib mvv2e in the order xx yy zz xy xz yz, each by fsum; also their magnitudes sum |term|"""
    m = np.asarray(mass, dtype=np.float64)
    K, mag = np.zeros(6), np.zeros(6)
    for c, (a, b) in enumerate(TENSOR):
        t = ((m * v[:, a] * v[:, b]) * MVV2E).tolist()
        K[c], mag[c] = math.fsum(t), math.fsum(abs(u) for u in t)
    return K, mag


def thermo(v, mass, ev, with_virial, tdof, volume, ecouple=0.0):
    """out[THERMO_N] of ani_md_thermo from the fsum sums"""
    K, _ = tensor_sums(v, mass)
    out = np.zeros(THERMO_N)
    k2 = K[0] + K[1] + K[2]
    pe, ke = float(ev[0]), 0.5 * k2
    out[0], out[1], out[2] = pe, ke, 2.0 * ke / (tdof * BOLTZ)
    if with_virial:
        out[3] = (k2 + ev[1] + ev[5] + ev[9]) / (3.0 * volume) * NKTV2P
        out[4:10] = [(K[c] + ev[W_INDEX[c]]) / volume * NKTV2P for c in range(6)]
    else:
        out[3:10] = np.nan
    out[10], out[11], out[12], out[13], out[14] = pe + ke, ecouple, pe + ke + ecouple, volume, k2
    return out


# ---- the scaled integrators (operation order of md_loop_reference, no fused multiply-adds) ------------------------------------
def scale(v, s):
    return v * s


def nh_initial_integrate(x, v, f, dtfm, dt, x_built, d2max, s):
    """v = s v;  v += dtfm f;  x += dt v;  returns (x, v, d2max)"""
    return mr.initial_integrate(x, scale(v, s), f, dtfm, dt, x_built, d2max)


def nh_final_integrate(v, f, dtfm, mass):
    """v += dtfm f;  returns (v, K2 of the new v by fsum)"""
    v, _ = mr.final_integrate(v, f, dtfm)
    return v, k2_sum(v, mass)


# ---- the trajectory ----------------------------------------------------------------------------------------------------------
def ramp_target(k, nsteps, t_start, t_stop):
    """target of step k = 1..nsteps of a run of nsteps"""
    return t_stop if k == nsteps else t_start + (k / nsteps) * (t_stop - t_start)


def nvt_trajectory(x0, v0, mass, evaluate, steps, dt, t_start, t_stop=None, t_period=None, M=3, nc=1, drag=0.0, tdof=None,
                   fresh_k2_every_step=True):
    """Thermostatted velocity Verlet in the order of VerletRun with set_nvt: chain half-step, v = s v, half kick, drift, forces, half
    kick, chain half-step, v = s v.  evaluate(x) -> (forces [n, 3], potential energy).  The chain starts at rest.
    fresh_k2_every_step: every step takes K2 from the velocities (step() N times); False: only the first (run(N)).
    Returns the records of step 0 .. steps: dicts of x, v, f, pe, ke, ecouple, t_target and chain (the state record)."""
    mass = np.asarray(mass, dtype=np.float64)
    n = len(mass)
    t_stop = t_start if t_stop is None else t_stop
    t_period = 100.0 * dt if t_period is None else t_period
    tdof = 3.0 * n - 3.0 if tdof is None else float(tdof)
    dtfm = (0.5 * dt * FTM2V) / mass
    x, v = np.array(x0, dtype=np.float64), np.array(v0, dtype=np.float64)
    eta, ed, edd = np.zeros(M), np.zeros(M), np.zeros(M)
    f, pe = evaluate(x)
    count, K2, s, ec, t = 0, k2_sum(v, mass), 1.0, 0.0, t_start

    def record():
        return dict(x=x.copy(), v=v.copy(), f=f.copy(), pe=float(pe), ke=0.5 * k2_sum(v, mass), ecouple=float(ec), t_target=t,
                    chain=state_record(count, K2, s, t, ec, tdof, 0, eta, ed, edd))

    out = [record()]
    for k in range(1, steps + 1):
        t = ramp_target(k, steps, t_start, t_stop)
        if fresh_k2_every_step or k == 1:
            K2 = k2_sum(v, mass)
        for half in range(2):
            if half == 1:
                K2 = k2_sum(v, mass)
            r = chain_half_step(K2, t, tdof, dt, t_period, drag, M, nc, eta, ed, edd)
            eta, ed, edd, s, K2, ec = r["eta"], r["eta_dot"], r["eta_dotdot"], float(r["s"]), float(r["K2"]), float(r["ecouple"])
            count += 1
            if half == 0:
                x, v, _ = nh_initial_integrate(x, v, f, dtfm, dt, x, 0.0, s)
                f, pe = evaluate(x)
                v, _ = nh_final_integrate(v, f, dtfm, mass)
            else:
                v = scale(v, s)
        out.append(record())
    return out


# ---- the 30-atom water box of the trajectory tests ---------------------------------------------------------------------------
WATER_MODEL = ("ani2x", 1, 2024)
T_START, T_TARGET, T_PERIOD, MTCHAIN = 300.0, 600.0, 20.0, 3


def water30(root):
    """(system, masses [30], start velocities: default_rng(300) at 300 K, momentum removed) of tests/golden/water-0.8nm.data"""
    import os
    from lammps_ani_amd import harness as hx
    s = hx.read_lammps_data(os.path.join(root, "tests", "golden", "water-0.8nm.data"))
    m = MASSES[s.types - 1]
    v = np.random.default_rng(300).normal(size=(s.natoms, 3)) * np.sqrt(BOLTZ * T_START / (m[:, None] * MVV2E))
    v -= (m[:, None] * v).sum(0) / m.sum()
    v.setflags(write=False)
    return s, m, v


def oracle_evaluator(model_path, sysm):
    """evaluate(x) -> (forces [n, 3] in global order, potential energy) by the CPU oracle on the periodic box of sysm"""
    from lammps_ani_amd import harness as hx
    from oracle import Oracle
    o, n, L = Oracle(model_path), sysm.natoms, sysm.boxhi - sysm.boxlo

    def evaluate(xx):
        xw = sysm.boxlo + np.mod(xx - sysm.boxlo, L)
        inp = hx.decompose(sysm, x_override=xw)
        r = o.compute(inp)
        f = np.zeros((n, 3))
        np.add.at(f, inp.tag[: inp.nlocal], r["force"][: inp.nlocal])
        np.add.at(f, inp.tag[inp.nlocal:], r["force"][inp.nlocal:])       # ghosts carry their owner's tag
        return f, float(r["energy"])

    return evaluate


def wander(a):
    a = np.asarray(a, dtype=np.float64)
    return float(a.max() - a.min())
