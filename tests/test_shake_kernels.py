"""GPU: the constraint kernels of include/ani_md.h (ani_md_shake_positions / ani_md_rattle_velocities) called directly through
ctypes, against the numpy RATTLE of tests/shake_reference.py.  No model.

Inputs (shake_reference.kernel_case, validated on the CPU by tests/test_shake_reference_cpu.py): nc clusters with K drawn from
{1, 2, 3} in random order, lengths from {0.96, 1.09, 1.01} A, centres C / N / O and partners H, centres uniform in a 20 A box,
partners exactly at d_k in random directions at least 60 degrees apart, everything wrapped into the box (cluster 0 is placed across
the +x face by hand), a quarter as many atoms in no cluster, v normal with sigma 0.05 A/fs, dt = 2 fs, x' = x0 + dt v.
Cluster counts 1, 63, 64, 65, 255, 256, 257 and 1500: a lone thread, wave edges, block edges, several blocks.

Bars.  tol = 1e-12, maxiter = 50: the residual bound leaves about tol d / 2 of position error (the numpy run of this recipe: 4.6e-13 A
over 1 500 clusters in at most 6 iterations), the bar is 100 tol max d, and the same divided by dt for v; the residual recomputed in
numpy from the device's x is at most tol + 1e-13 (the 1e-13: rounding of 20 A coordinates).  tol = 1e-4, maxiter = 20 (the
reference's input): residual at most tol, max |x - x_ref| <= tol max d (numpy: 0.47e-4 d).  Velocity stage: |r . (v_c - v_p)| <=
1e-12 |r| max |v| and v within 1e-12 max |v| of the reference (the 3 x 3 system has a condition number below about 20 at these
angles: far above rounding).
"""
import numpy as np
import pytest

import shake_reference as sr

pytestmark = pytest.mark.gpu

COUNTS = pytest.mark.parametrize("nc", sr.KERNEL_COUNTS)
PMASK = 7


@pytest.fixture(scope="module")
def hip():
    from lammps_ani_amd import ani_hip
    return ani_hip


class Device:
    """the arrays of one case on the card and the two stages on them"""

    def __init__(self, hip, case, x, v, d=None):
        import torch
        self.torch, self.lib = torch, hip.lib()
        dev = torch.device("cuda:0")
        t = lambda a: torch.as_tensor(np.array(a, dtype=np.float64), device=dev)
        self.x, self.v, self.w, self.xb = t(x), (None if v is None else t(v)), t(case["w"]), t(case["x0"])
        self.d = t(case["d"] if d is None else d)
        self.cl = torch.as_tensor(np.ascontiguousarray(case["cl"], dtype=np.int32), device=dev).clone()
        self.nc = int(case["cl"].shape[0])
        self.len3 = np.ascontiguousarray(case["L"], dtype=np.float64)
        self.d2max = torch.zeros(1, dtype=torch.float64, device=dev)
        self.stats = torch.zeros(hip.SHAKE_NSTATS, dtype=torch.int64, device=dev)

    def shake(self, tol, maxiter, dt=sr.DT):
        rc = self.lib.ani_md_shake_positions(self.x.data_ptr(), None if self.v is None else self.v.data_ptr(), self.cl.data_ptr(),
                                             self.d.data_ptr(), self.nc, self.w.data_ptr(), dt, tol, maxiter, self.len3.ctypes.data,
                                             PMASK, self.xb.data_ptr(), self.d2max.data_ptr(), self.stats.data_ptr(), None)
        assert rc == 0

    def rattle(self):
        rc = self.lib.ani_md_rattle_velocities(self.x.data_ptr(), self.v.data_ptr(), self.cl.data_ptr(), self.d.data_ptr(), self.nc,
                                               self.w.data_ptr(), self.len3.ctypes.data, PMASK, None)
        assert rc == 0

    def read(self):
        self.torch.cuda.synchronize()
        st = self.stats.cpu().numpy().view(np.uint64)
        rec = dict(unconverged=int(st[0]), max_iterations=int(st[1]), max_residual=float(st[2:3].view(np.float64)[0]), calls=int(st[3]))
        return self.x.cpu().numpy(), (None if self.v is None else self.v.cpu().numpy()), rec, float(self.d2max.cpu()[0])


def _shake(hip, case, tol, maxiter):
    d = Device(hip, case, case["xp"], case["v"])
    d.shake(tol, maxiter)
    return d.read()


@COUNTS
def test_position_stage_to_a_tight_tolerance(nc, hip):
    tol = 1e-12
    case, xr, vr, it, _ = sr.kernel_case_reference(nc)
    assert len(case["straddling"]) >= 1                                  # at least one cluster sits across a face
    x, v, st, d2 = _shake(hip, case, tol, 50)
    dmax = case["d"].max()
    ex, ev_ = np.abs(x - xr).max(), np.abs(v - vr).max()
    res = sr.residuals(x, case["cl"], case["d"], case["L"]).max()
    print(f"nc {nc}: max |dx| {ex:.2e} A  |dv| {ev_:.2e} A/fs  residual {res:.2e} (device says {st['max_residual']:.2e})  "
          f"iterations {st['max_iterations']} (numpy to 1e-15: {it.max()})  straddling {len(case['straddling'])}")
    assert ex <= 100 * tol * dmax
    assert ev_ <= 100 * tol * dmax / sr.DT
    assert res <= tol + 1e-13
    assert st["unconverged"] == 0 and st["max_iterations"] <= 10 and st["calls"] == 1
    assert 0.0 <= st["max_residual"] <= tol
    # atoms in no cluster: bitwise what they were
    free = case["free"]
    assert x[free].tobytes() == case["xp"][free].tobytes() and v[free].tobytes() == case["v"][free].tobytes()
    # the displacement maximum over the moved atoms, against x_built = x0
    ref = ((x[case["moved"]] - case["x0"][case["moved"]]) ** 2).sum(1).max()
    assert abs(d2 - ref) <= 1e-13 * ref
    # a second launch on the same inputs: bitwise the same outputs
    x2, v2, st2, d22 = _shake(hip, case, tol, 50)
    assert x2.tobytes() == x.tobytes() and v2.tobytes() == v.tobytes() and st2 == st and d22 == d2


@COUNTS
def test_position_stage_at_the_tolerance_of_the_reference_input(nc, hip):
    tol = 1e-4                                                            # fix shake 0.0001 20
    case, xr, vr, _, _ = sr.kernel_case_reference(nc)
    x, v, st, _ = _shake(hip, case, tol, 20)
    res = sr.residuals(x, case["cl"], case["d"], case["L"]).max()
    ex = np.abs(x - xr).max()
    print(f"nc {nc}: residual {res:.3e}  max |dx| {ex:.3e} A = {ex / case['d'].max():.3e} d  iterations {st['max_iterations']}")
    assert res <= tol
    assert ex <= tol * case["d"].max()
    assert st["unconverged"] == 0 and st["max_iterations"] <= 10


@COUNTS
def test_one_iteration_is_counted_as_unconverged_and_stays_finite(nc, hip):
    case = sr.kernel_case(nc)
    x, v, st, d2 = _shake(hip, case, 1e-12, 1)
    _, _, it, res = sr.shake_positions(case["xp"], case["v"], case["cl"], case["d"], case["w"], sr.DT, case["L"], tol=1e-12, maxiter=1)
    assert st["unconverged"] > 0 and st["unconverged"] == int((res > 1e-12).sum()) and st["max_iterations"] == 1
    assert np.isfinite(x).all() and np.isfinite(v).all() and np.isfinite(st["max_residual"]) and np.isfinite(d2)
    assert st["max_residual"] > 1e-12


def test_statistics_accumulate_over_calls(hip):
    case = sr.kernel_case(257)
    d = Device(hip, case, case["xp"], case["v"])
    d.shake(1e-12, 1)
    _, _, st1, _ = d.read()
    d.x.copy_(d.torch.as_tensor(case["xp"]))
    d.v.copy_(d.torch.as_tensor(case["v"]))
    d.shake(1e-12, 1)
    _, _, st2, _ = d.read()
    assert st2["calls"] == 2 and st2["unconverged"] == 2 * st1["unconverged"] and st2["max_residual"] == st1["max_residual"]


@COUNTS
def test_velocity_stage(nc, hip):
    case, xr, vr, _, vrat = sr.kernel_case_reference(nc)
    d = Device(hip, case, xr, vr)
    d.rattle()
    x, v, _, _ = d.read()
    vmax = np.abs(vrat).max()
    defect, err = sr.velocity_defect(xr, v, case["cl"], case["L"]), np.abs(v - vrat).max()
    print(f"nc {nc}: largest |r . dv| / |r| {defect:.2e}  max |v - v_ref| {err:.2e}  (max |v| {vmax:.2e}; before the stage "
          f"{sr.velocity_defect(xr, vr, case['cl'], case['L']):.2e})")
    assert defect <= 1e-12 * vmax
    assert err <= 1e-12 * vmax
    assert x.tobytes() == xr.tobytes()                                    # positions are read only
    assert v[case["free"]].tobytes() == vr[case["free"]].tobytes()
    d2 = Device(hip, case, xr, vr)
    d2.rattle()
    assert d2.read()[1].tobytes() == v.tobytes()


@COUNTS
def test_the_form_without_velocities_projects_a_start_configuration(nc, hip):
    """v == NULL: old and new positions are the same, no velocity is written"""
    tol = 1e-12
    case = sr.kernel_case(nc)
    lengths = case["d"] * 1.02
    xr, _, it, _ = sr.shake_positions(case["x0"], None, case["cl"], lengths, case["w"], sr.DT, case["L"])
    d = Device(hip, case, case["x0"], None, d=lengths)
    keep = d.torch.as_tensor(case["v"], device=d.x.device).clone()        # a velocity array beside it: nobody knows it
    d.shake(tol, 50)
    x, _, st, _ = d.read()
    assert np.abs(x - xr).max() <= 100 * tol * lengths.max()
    assert sr.residuals(x, case["cl"], lengths, case["L"]).max() <= tol + 1e-13
    assert st["unconverged"] == 0 and 1 <= st["max_iterations"] <= 10
    assert keep.cpu().numpy().tobytes() == case["v"].tobytes()
    assert x[case["free"]].tobytes() == case["x0"][case["free"]].tobytes()
    # on a configuration that holds already: no iteration, nothing moves
    d.stats.zero_()
    d.shake(tol + 1e-13, 50)
    x2, _, st2, _ = d.read()
    assert st2["max_iterations"] == 0 and x2.tobytes() == x.tobytes()
