"""GPU: image flags, mean-squared displacements and trajectory frames in the timestep loop (VerletRun.set_images / set_msd /
set_dump: the kernels of include/ani_md_transport.h), on the reference's 30-atom water box, tests/golden/water-0.8nm.data.

(i) Elementwise calculator (tests/test_shake_md.py: the atoms do not interact, the same positions give the same bits), dt 0.5 fs,
every = 2, skin 2 A, velocities +-0.4 A/fs in every component with the sign alternating with the tag, 60 steps: every atom crosses
a face (12 A in a box of 8 A), the displacement check re-neighbours every few steps.  The reference is a NumPy velocity Verlet of
the same force law that never wraps (the force is periodic): the two runs differ only by the rounding of wrapped against unwrapped
storage, about 4e-15 A per step, and the stiffest atom (a hydrogen: omega^2 = 30 * 2 pi / L * ftm2v / m, omega ~ 0.1 / fs) amplifies
that by at most e^3 over 30 fs -- the bar of 1e-10 A is far above it and far below anything an image flag could get wrong (8 A).
(ii) The model, both precisions: 300 K plus a uniform drift of (0.4, -0.4, 0.4) A/fs, 20 steps with a forced rebuild every fifth.
(iii) The dump: a DCD file and the kept frames against unwrapped_positions() at the frames' steps.
(iv) Clearing, minimize, the barostat's box, and the refusals.
"""
import functools
import os

import numpy as np
import pytest

import nh_reference as nh
import transport_reference as tr
from test_npt_md import NPT
from test_nvt_md import _loop
from test_shake_md import _Recorder, _periodic_forces

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, STEPS, SPEED, STRIDE = 0.5, 60, 0.4, 3
FTM2V = 1.0 / 48.88821291 / 48.88821291
GROUPS = {"all": None, "O": "O", "H": "H"}
DRIFT = np.array([0.4, -0.4, 0.4])
PRECISIONS = pytest.mark.parametrize("single", [True, False], ids=["precision_single", "precision_double"])


def _start_velocities(n):
    """+-0.4 A/fs in every component, the sign alternating with the tag: [n, 3] by tag"""
    return SPEED * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None] * np.ones(3)


@functools.lru_cache(maxsize=None)
def _unwrapped_reference():
    """velocity Verlet with f = 30 sin(2 pi (x - lo) / L + tag) and no wrapping, the loop's arithmetic (dtfm = dt / 2 * ftm2v / m):
    (xu [STEPS + 1, n, 3], rebuilds that the loop's displacement rule makes on this trajectory)"""
    s, m, _ = nh.water30(ROOT)
    lo, L = s.boxlo, s.boxhi - s.boxlo
    phase = np.arange(s.natoms, dtype=np.float64)[:, None]
    dtfm = (0.5 * DT * FTM2V / m)[:, None]

    def force(x):
        return 30.0 * np.sin(2.0 * np.pi * (x - lo) / L + phase)

    x, v = s.x.copy(), _start_velocities(s.natoms)
    f = force(x)
    traj, built, since, rebuilds = [x.copy()], x.copy(), 0, 0
    for _ in range(STEPS):
        v = v + dtfm * f
        x = x + DT * v
        since += 1
        if since % 2 == 0 and ((x - built) ** 2).sum(1).max() > 1.0:      # every = 2, (skin / 2)^2
            built, since, rebuilds = x.copy(), 0, rebuilds + 1
        f = force(x)
        v = v + dtfm * f
        traj.append(x.copy())
    return np.array(traj), rebuilds


def _cells(xu, s):
    return np.floor((xu - s.boxlo) / (s.boxhi - s.boxlo)).astype(np.int64)


def test_the_start_exercises_every_face_on_the_cpu():
    """the exclusion cap of (i), from the NumPy integrator alone: every (dimension, sign) has an atom that ends in another cell
    than it started in, the displacement rule re-neighbours at least three times, and no coordinate moves more than 0.5 A a step"""
    s, _, _ = nh.water30(ROOT)
    traj, rebuilds = _unwrapped_reference()
    moved = _cells(traj[-1], s) - _cells(traj[0], s)
    for k in range(3):
        assert (moved[:, k] > 0).any() and (moved[:, k] < 0).any()
    assert rebuilds >= 3
    assert np.abs(np.diff(traj, axis=0)).max() < 0.5


def _elementwise_loop(model_cache, **kw):
    import torch
    s, _, _ = nh.water30(ROOT)
    run, ani, glob = _loop(model_cache(*nh.WATER_MODEL), True, velocities=False, **kw)
    _periodic_forces(run, s)
    run.v.copy_(torch.as_tensor(_start_velocities(s.natoms)[run.tag.cpu().numpy()]))
    return run, ani, glob, s


def _by_group(s):
    species = np.asarray(s.types) - 1                     # ANI-2x order H C N O ...
    return {"all": np.ones(s.natoms, bool), "O": species == 3, "H": species == 0}


def _check_msd(got, xu, x0u, mass, members, what):
    ref, terms = tr.msd(xu, x0u, mass, members)
    bound = tr.msd_bounds(terms)
    row = np.concatenate([got["msd"], got["msd_com"], got["dcm"], [got["nonfinite"]]])
    err = np.abs(row - ref)
    print(f"{what}: msd {got['msd'][3]:.6f} com {got['msd_com'][3]:.6e} A^2; |error| max {err.max():.2e}, largest error / bound "
          f"{(err[:11] / bound[:11]).max():.3f}")
    assert got["count"] == terms["N"] and (err <= bound).all(), (what, err, bound)


@pytest.fixture(scope="module")
def stepped(model_cache):
    """60 step() calls of (i) with everything read back at every step"""
    run, ani, glob, s = _elementwise_loop(model_cache)
    run.set_msd(GROUPS, stride=STRIDE)
    builds0 = run.nbuilds
    origin = run.unwrapped_positions()
    xu, xw = [origin], [glob(run.x)]
    for _ in range(STEPS):
        run.step()
        xu.append(run.unwrapped_positions())
        xw.append(glob(run.x))
    out = dict(s=s, xu=np.array(xu), xw=np.array(xw), images=run.images(), msd=run.msd(), series=run.msd_series(),
               rebuilds=run.nbuilds - builds0, origin=origin)
    ani.close()
    return out


def test_images_cover_every_face_and_unwrapped_positions_are_continuous(stepped):
    s, img = stepped["s"], stepped["images"]
    for k in range(3):
        assert (img[:, k] > 0).any() and (img[:, k] < 0).any(), (k, img[:, k])          # the exclusion cap
    assert stepped["rebuilds"] >= 3
    du, dw = np.abs(np.diff(stepped["xu"], axis=0)), np.abs(np.diff(stepped["xw"], axis=0))
    L = s.boxhi - s.boxlo
    print(f"rebuilds {stepped['rebuilds']}; largest step of an unwrapped coordinate {du.max():.3f} A, of a wrapped one {dw.max():.3f} A")
    assert du.max() <= 0.5
    assert (dw.max(axis=(0, 1)) > L - 0.5).all()                                         # the wrapped ones jump by a box length
    assert (stepped["xu"][0] == stepped["xw"][0]).all()                                 # images count from set_images


def test_unwrapped_positions_follow_the_reference_that_never_wraps(stepped):
    traj, _ = _unwrapped_reference()
    err = np.abs(stepped["xu"] - traj).max(axis=(1, 2))
    print(f"|xu - reference| after 1, 10, 30, 60 steps: {err[1]:.2e} {err[10]:.2e} {err[30]:.2e} {err[60]:.2e} A")
    assert err[-1] <= 1e-10 and err.max() <= 1e-10
    assert (_cells(traj[-1], stepped["s"]) - _cells(traj[0], stepped["s"]) != 0).any(axis=0).all()


def test_msd_of_the_loop_and_its_series(stepped):
    s, m = stepped["s"], nh.water30(ROOT)[1]
    for name, members in _by_group(s).items():
        _check_msd(stepped["msd"][name], stepped["xu"][-1], stepped["origin"], m, members, name)
    assert stepped["msd"]["O"]["count"] == 10 and stepped["msd"]["H"]["count"] == 20
    ser = stepped["series"]
    assert ser["step"].tolist() == list(range(STRIDE, STEPS + 1, STRIDE)) and ser["dropped"] == 0
    for g, name in enumerate(GROUPS):
        last = stepped["msd"][name]
        assert ser["groups"][name]["msd"][-1].tobytes() == last["msd"].tobytes()
        assert ser["groups"][name]["msd_com"][-1].tobytes() == last["msd_com"].tobytes()
        assert ser["groups"][name]["dcm"][-1].tobytes() == last["dcm"].tobytes()
        for r, step in enumerate(ser["step"].tolist()):                                   # every row is the MSD of its own step
            ref, terms = tr.msd(stepped["xu"][step], stepped["origin"], m, _by_group(s)[name])
            assert (np.abs(ser["rows"][r, g] - ref) <= tr.msd_bounds(terms)).all(), (name, step)


def test_run_gives_the_images_and_the_series_of_steps(stepped, model_cache):
    run, ani, _, _ = _elementwise_loop(model_cache)
    run.set_msd(GROUPS, stride=STRIDE)
    run.run(STEPS)
    assert (run.images() == stepped["images"]).all()
    ser = run.msd_series()
    assert ser["step"].tolist() == stepped["series"]["step"].tolist()
    assert ser["rows"].tobytes() == stepped["series"]["rows"].tobytes()
    assert run.unwrapped_positions().tobytes() == stepped["xu"][-1].tobytes()
    # a series that wraps: capacity 4, the last four rows in time order, the rest counted as dropped
    run.set_msd(GROUPS, stride=1, capacity=4)
    run.run(6)
    ser = run.msd_series(reset=True)
    assert ser["step"].tolist() == [STEPS + 3, STEPS + 4, STEPS + 5, STEPS + 6] and ser["dropped"] == 2
    assert run.msd_series()["step"].size == 0
    ani.close()


@PRECISIONS
def test_model_run_with_a_drift(single, model_cache):
    import torch
    s, m, v0 = nh.water30(ROOT)
    run, ani, glob = _loop(model_cache(*nh.WATER_MODEL), single, velocities=False)
    run.v.copy_(torch.as_tensor((v0 + DRIFT)[run.tag.cpu().numpy()]))
    run.set_msd(GROUPS)
    origin = run.unwrapped_positions()
    for k in range(20):
        run.step(force_rebuild=(k % 5 == 4))
    img, xu, got = run.images(), run.unwrapped_positions(), run.msd()
    for k in range(3):
        assert (img[:, k] != 0).sum() >= 5, (k, img[:, k])                                # the exclusion cap
        assert (np.sign(img[:, k][img[:, k] != 0]) == np.sign(DRIFT[k])).all()
    t = 20 * DT
    print(f"dcm of all atoms {got['all']['dcm']} against drift * t {DRIFT * t}; msd com yes {got['all']['msd_com'][3]:.6f} A^2")
    assert np.abs(got["all"]["dcm"] - DRIFT * t).max() <= 1e-9
    for name, members in _by_group(s).items():
        _check_msd(got[name], xu, origin, m, members, f"{'fp32' if single else 'fp64'} handle, {name}")
    assert got["O"]["count"] == 10 and got["H"]["count"] == 20 and got["all"]["count"] == 30
    assert all(g["nonfinite"] == 0 for g in got.values())
    assert 0.0 < got["all"]["msd_com"][3] < 1.0 < got["all"]["msd"][3]                   # thermal motion against 48 A^2 of drift
    ani.close()


def test_dump_to_a_dcd_file_and_to_kept_frames(model_cache, tmp_path):
    import torch
    s, _, v0 = nh.water30(ROOT)
    L = s.boxhi - s.boxlo
    path = str(tmp_path / "water.dcd")
    results = []
    for target in (path, None):
        run, ani, _ = _loop(model_cache(*nh.WATER_MODEL), True, velocities=False)
        run.v.copy_(torch.as_tensor((v0 + DRIFT)[run.tag.cpu().numpy()]))
        run.set_dump(every=2, path=target, unwrap=True, capacity=3)
        seen, drained = {}, []

        def after(k, run=run, seen=seen, drained=drained):
            if run.step_no % 2 == 0:
                seen[run.step_no] = np.float32(run.unwrapped_positions())
            drained.append(run._dump["nring"])

        run.run(10, after_forces=after)
        assert drained == [0, 1, 1, 2, 2, 0, 0, 1, 1, 2]                                   # the ring of three was drained mid-run
        if target is None:
            fr = run.frames()
            assert run.frames()["step"].size == 0                                         # reset
            run.set_dump(0)
        else:
            assert run.frames()["step"].size == 0                                         # they are in the file
            run.set_dump(0)
            got = tr.read_dcd(path)
            assert got["nset"] == 5 and got["first_step"] == 2 and got["every"] == 2 and got["last_step"] == 10
            assert got["natoms"] == 30 and got["dt"] == np.float32(DT)
            assert got["size"] == 276 + 5 * (56 + 3 * (4 * 30 + 8))
            fr = dict(step=got["first_step"] + got["every"] * np.arange(got["nset"]), xyz=got["xyz"],
                      cell=np.concatenate([np.broadcast_to(s.boxlo, (5, 3)), got["cell"]], axis=1))
        assert run._dump is None
        assert fr["step"].tolist() == [2, 4, 6, 8, 10] == sorted(seen)
        assert fr["cell"].tobytes() == np.tile(np.concatenate([s.boxlo, L]), (5, 1)).tobytes()
        assert fr["xyz"].dtype == np.float32 and fr["xyz"].shape == (5, 30, 3)
        for f, step in enumerate(fr["step"].tolist()):
            assert fr["xyz"][f].tobytes() == seen[step].tobytes(), step
        moved = np.abs(fr["xyz"][-1] - fr["xyz"][0])                                      # unwrapped: 4 fs of drift, 1.6 A, no jump
        assert (moved.max(axis=0) > 1.0).all() and moved.max() < 3.0
        results.append(fr)
        ani.close()
    # wrapped frames: what the loop holds, fp32, by tag
    run, ani, glob = _loop(model_cache(*nh.WATER_MODEL), True)
    run.set_dump(every=1, capacity=2)
    run.step(force_rebuild=True)
    fr = run.close_dump()
    assert fr["step"].tolist() == [1] and fr["xyz"][0].tobytes() == np.float32(glob(run.x)).tobytes()
    ani.close()


CLEARED = ["initial_integrate", "check", "final_integrate",
           "initial_integrate", "wrap_positions", "ghost_shell_count", "ghost_shell_fill", "append_ghosts", "check", "final_integrate",
           "initial_integrate", "check", "final_integrate"]


def _trace(run):
    calls = []
    md = run._md
    run._md = _Recorder(md, calls)
    for k in range(3):
        run.step(force_rebuild=(k == 1))
    run._md = md
    return [c[len("ani_md_"):] for c in calls]


def test_cleared_features_leave_the_launches_of_a_loop_that_never_had_them(model_cache):
    path = model_cache(*nh.WATER_MODEL)
    run, ani, _ = _loop(path, True, every=1)
    plain = _trace(run)
    ani.close()
    assert plain == CLEARED
    run, ani, _ = _loop(path, True, every=1)
    run.set_msd(GROUPS, stride=1)
    run.set_dump(1)
    with pytest.raises(RuntimeError, match="MSD or a dump"):
        run.set_images(False)
    on = _trace(run)
    want = [c.replace("wrap_positions", "wrap_positions_images") for c in plain]
    extra = ["msd_sample", "frame_pack"]
    assert [c for c in on if c not in extra] == want
    assert on.count("msd_sample") == 3 and on.count("frame_pack") == 3
    run.set_msd({})
    run.set_dump(0)
    assert _trace(run) == want                      # images on: the wrap that counts in place of the wrap, nothing else
    run.set_images(False)
    assert _trace(run) == plain
    for reader in (run.images, run.unwrapped_positions, run.msd, run.msd_series, run.frames, run.reset_msd_origin):
        with pytest.raises(RuntimeError, match="set_images|set_msd|set_dump"):
            reader()
    ani.close()


def test_minimize_keeps_the_images_and_writes_no_row(model_cache):
    import torch
    s, _, _ = nh.water30(ROOT)
    run, ani, _ = _loop(model_cache(*nh.WATER_MODEL), True, velocities=False, every=100)
    run.v.copy_(torch.as_tensor(np.broadcast_to(DRIFT, (30, 3)).copy()))
    run.set_msd(GROUPS, stride=1)
    run.run(5)                                      # 1 A per component and no look: atoms stand outside the box, unwrapped
    assert not run.images().any() and run.msd_series()["step"].tolist() == [1, 2, 3, 4, 5]
    before = run.unwrapped_positions()
    out = run.minimize(0.0, 0.0, 6, check_every=2)
    after, img = run.unwrapped_positions(), run.images()
    print(f"minimize: {out['iterations']} iterations, {out['rebuilds']} rebuilds, {int((img != 0).sum())} image flags set, "
          f"largest move {np.abs(after - before).max():.3f} A")
    assert out["rebuilds"] >= 1 and img.any()
    assert np.abs(after - before).max() <= out["iterations"] * 0.15      # dmax = 0.1 A a move, half a move back at an uphill event
    assert run.msd_series()["step"].tolist() == [1, 2, 3, 4, 5]          # minimize() does not sample
    ani.close()


def test_under_the_barostat_the_box_comes_from_the_record(model_cache):
    import torch
    _, _, v0 = nh.water30(ROOT)
    run, ani, glob = _loop(model_cache(*nh.WATER_MODEL), False, velocities=False, vflag=True)
    # image flags from four drifting steps in the box at rest (under the thermostat a drift would count as heat and be braked), then
    # the start velocities of tests/test_npt_md.py and its barostat: the flags now multiply a box that moves
    tag = run.tag.cpu().numpy()
    run.set_images()
    run.v.copy_(torch.as_tensor((v0 + 2.0 * DRIFT)[tag]))
    for _ in range(4):
        run.step(force_rebuild=True)
    flags = run.images()
    run.v.copy_(torch.as_tensor(np.array(v0[tag])))
    run.set_npt(nh.T_TARGET, **NPT)
    run.set_dump(every=1, unwrap=True, capacity=8)
    for _ in range(4):
        run.step(force_rebuild=True)
    xu, img, st = run.unwrapped_positions(), run.images(), run.npt_state()
    assert (flags != 0).sum() >= 5 and (img != 0).sum() >= 5
    assert not np.array_equal(st["len"], nh.water30(ROOT)[0].boxhi - nh.water30(ROOT)[0].boxlo)
    want = glob(run.x) + img.astype(np.float64) * st["len"]
    assert xu.tobytes() == want.tobytes()
    fr = run.frames()
    assert fr["step"].tolist() == [5, 6, 7, 8]
    assert fr["cell"][-1].tobytes() == np.concatenate([st["lo"], st["len"]]).tobytes()
    assert fr["xyz"][-1].tobytes() == np.float32(want).tobytes()
    assert (np.diff(fr["cell"][:, 3]) != 0).all()                        # every frame has the box of its own moment
    ani.close()


def test_where_it_raises(model_cache, monkeypatch):
    path = model_cache(*nh.WATER_MODEL)
    run, ani, _ = _loop(path, True)
    with pytest.raises(ValueError, match="at most 8"):
        run.set_msd({f"g{k}": None for k in range(9)})
    with pytest.raises(ValueError, match="at most 16 classes"):
        run.set_msd({f"bit{b}": [t for t in range(30) if (t >> b) & 1] for b in range(5)})
    with pytest.raises(ValueError, match="unknown species 'Xe'"):
        run.set_msd({"a": "Xe"})
    with pytest.raises(ValueError, match=r"unknown tag 999\b"):
        run.set_msd({"a": [0, 999]})
    with pytest.raises(ValueError, match="stride"):
        run.set_msd(GROUPS, stride=-1)
    with pytest.raises(ValueError, match="capacity"):
        run.set_msd(GROUPS, capacity=0)
    with pytest.raises(ValueError, match="capacity"):
        run.set_dump(1, capacity=0)
    with pytest.raises(ValueError, match="every"):
        run.set_dump(-1)
    assert run._msd is None and run._dump is None and run._img is None
    run.set_msd({"odd": np.arange(1, 30, 2), "water O": ["O"], "both": ["O", "H"]})
    assert [g["count"] for g in run.msd().values()] == [15, 10, 30]
    with pytest.raises(RuntimeError, match="MSD or a dump"):
        run.set_images(False)
    run.set_msd({})
    run.set_images(False)
    monkeypatch.setattr(run.dc, "multi", True)                            # what a loop on two ranks, or force_collectives, sees
    for setter in (run.set_images, lambda: run.set_msd(GROUPS), lambda: run.set_dump(1)):
        with pytest.raises(RuntimeError, match="one rank only"):
            setter()
    ani.close()
    monkeypatch.setenv("ANI_MD_NATIVE_REBUILD", "0")
    run, ani, _ = _loop(path, True)
    for setter in (run.set_images, lambda: run.set_msd(GROUPS), lambda: run.set_dump(1)):
        with pytest.raises(RuntimeError, match="native re-neighbouring"):
            setter()
    ani.close()
