"""GPU: RDF sampling in the timestep loop (VerletRun.set_rdf / sample_rdf / rdf: one ani_rdf_accumulate_device launch behind the force
evaluation of every `every`-th step) against the brute-force reference tests/rdf_reference.py on positions read back from the loop.

The reference's 30-atom water box (tests/golden/water-0.8nm.data, 8 A wide: most neighbours inside 5.1 A are images), velocities at
300 K, O-O, O-H, H-O, H-H with 48 bins to the force cutoff, a frame every second step, six steps with a forced re-neighbouring on
step 3.  Integer counts: every comparison is an equality.  The sampled positions are the loop's own, so the test measures on them how
far any pair lies from a bin edge and fails as inconclusive, naming the seed to change, if that is ever below the bar."""
import os

import numpy as np
import pytest

import rdf_reference as rr
from lammps_ani_amd import harness as hx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("O", "O"), ("O", "H"), ("H", "O"), ("H", "H")]
PAIR_IDX = [(3, 3), (3, 0), (0, 3), (0, 0)]     # ANI-2x species order H C N O S F Cl
NBINS, RMAX, SEED, DT = 48, 5.1, 12345, 0.5
GAP = 1e-9
PRECISIONS = pytest.mark.parametrize("single", [True, False], ids=["precision_single", "precision_double"])


def _system():
    return hx.read_lammps_data(os.path.join(ROOT, "tests", "golden", "water-0.8nm.data"))


def _loop(model_cache, single, rdf=True):
    import torch
    from lammps_ani_amd import ani_hip, md
    sysm = _system()
    ani = ani_hip.ANI(model_cache("ani2x", 1, 11), 0, -1, use_single=single)
    run = md.VerletRun(ani, hx.decompose(sysm), sysm.boxhi - sysm.boxlo, torch.device("cuda:0"), dt=DT, box_lo=sysm.boxlo, every=2,
                       seed=SEED)
    run.create_velocities(300.0)
    if rdf:
        run.set_rdf(PAIRS, nbins=NBINS, every=2)
    return run, ani, sysm


def _frame(run, sysm):
    """the loop's owned positions of this moment as a whole periodic box for the reference"""
    n = run.nlocal
    assert n == sysm.natoms
    tag = run.tag.cpu().numpy()
    return hx.System(run.x[:n].cpu().numpy().copy(), sysm.types[tag], sysm.boxlo, sysm.boxhi)


def _six_steps(run, sysm):
    """six step() calls, re-neighbouring forced on step 3: the reference's sum over the three sampled frames, their smallest edge
    gap, and the last frame's own counts"""
    total = np.zeros((len(PAIRS), NBINS), dtype=np.uint64)
    gap, last = np.inf, None
    nb = run.nbuilds
    for k in range(1, 7):
        run.step(force_rebuild=(k == 3))
        if k % 2 == 0:
            last, _, g = rr.scan(_frame(run, sysm), PAIR_IDX, NBINS, RMAX)
            total += last
            gap = min(gap, g)
    assert run.nbuilds >= nb + 1
    return total, gap, last


def _inconclusive(gap, bar):
    print("smallest edge gap of the sampled frames", gap)
    if not gap > bar:
        pytest.fail(f"inconclusive: a pair of a sampled frame lies {gap:.3e} A from a bin edge (bar {bar:.0e}); change SEED = {SEED}")


@PRECISIONS
def test_sampled_steps_equal_the_reference(single, model_cache):
    run, ani, sysm = _loop(model_cache, single)
    assert run.rdf()["frames"] == 0
    total, gap, last = _six_steps(run, sysm)
    _inconclusive(gap, GAP)
    out = run.rdf()
    n_o, n_h = int((sysm.types == 4).sum()), int((sysm.types == 1).sum())
    print("totals", out["counts"].sum(1).tolist(), "reference", total.sum(1).tolist())
    assert out["frames"] == 3
    assert out["centres"].tolist() == [3 * n_o, 3 * n_o, 3 * n_h, 3 * n_h]
    # the frames are not empty: an ideal gas of this density has N (N - 1) / V * 4 pi / 3 rmax^3 ordered pairs inside rmax per frame
    ideal = 3 * sysm.natoms * (sysm.natoms - 1) / float(np.prod(sysm.boxhi - sysm.boxlo)) * 4.0 * np.pi / 3.0 * RMAX ** 3
    assert abs(float(total.sum()) / ideal - 1.0) < 0.2
    assert np.array_equal(out["counts"], total)
    assert np.array_equal(out["counts"][1].sum(), out["counts"][2].sum())      # O-H and H-O are mirrors
    # normalised like compute rdf
    from lammps_ani_amd import ani_hip
    L = sysm.boxhi - sysm.boxlo
    want = ani_hip.rdf_normalise(total, out["centres"], NBINS, RMAX, PAIR_IDX, np.bincount(sysm.types - 1, minlength=7), float(np.prod(L)))
    for k in ("r", "g", "coord"):
        assert np.array_equal(out[k], want[k])
    # sample_rdf: one more frame, on the positions as they are (those of step 6)
    run.sample_rdf()
    out = run.rdf()
    assert out["frames"] == 4 and np.array_equal(out["counts"], total + last)
    # reset keeps the configuration
    assert run.rdf(reset=True)["frames"] == 4
    out = run.rdf()
    assert out["frames"] == 0 and not out["counts"].any() and not out["centres"].any()
    run.step()
    run.step()
    assert run.rdf()["frames"] == 1
    ani.close()


@PRECISIONS
def test_run_samples_like_step(single, model_cache):
    """run(6) from the same start: the same counts as six step() calls.  The two trajectories differ by the order of the fp32 force
    sums and by the forced re-neighbouring (some 1e-8 A after six steps), hence the wider bar on the gap here."""
    run, ani, sysm = _loop(model_cache, single)
    total, gap, _ = _six_steps(run, sysm)
    _inconclusive(gap, 1e-7)
    by_step = run.rdf()
    ani.close()
    run, ani, sysm = _loop(model_cache, single)
    run.run(6)
    by_run = run.rdf()
    assert by_run["frames"] == by_step["frames"] == 3
    assert np.array_equal(by_run["centres"], by_step["centres"])
    assert np.array_equal(by_step["counts"], total) and np.array_equal(by_run["counts"], total)
    ani.close()


def test_clearing_restores_the_loop_and_minimize_does_not_sample(model_cache):
    from lammps_ani_amd import ani_hip
    run, ani, sysm = _loop(model_cache, True)
    run.step()
    run.step()
    assert run.rdf()["frames"] == 1
    run.set_rdf([])
    run.step()          # a loop that still sampled would raise here: nothing is configured
    run.step()
    with pytest.raises(RuntimeError, match="no RDF is set"):
        run.rdf()
    with pytest.raises(RuntimeError, match="no RDF is set"):
        run.sample_rdf()
    with pytest.raises(ani_hip.AniError, match="nothing is configured"):
        ani.rdf_read()
    # accumulators configured on the handle behind the loop's back: a cleared loop does not touch them
    ani.rdf_configure(NBINS, RMAX, PAIRS)
    run.step()
    run.step()
    counts, centres, frames = ani.rdf_read()
    assert frames == 0 and not counts.any() and not centres.any()
    # minimize() with an RDF set does not sample
    run.set_rdf(PAIRS, nbins=NBINS, every=1)
    run.step()
    assert run.rdf()["frames"] == 1
    res = run.minimize(0.0, 1e-3, 6)
    assert res["force_evaluations"] >= 6
    out = run.rdf()
    assert out["frames"] == 1
    before = out["counts"].copy()
    run.step()
    out = run.rdf()
    assert out["frames"] == 2 and out["counts"].sum() > before.sum()
    # a refused configuration changes nothing: what was set goes on
    with pytest.raises(ani_hip.AniError, match="rmax"):
        run.set_rdf(PAIRS, rmax=6.0)
    with pytest.raises(ValueError, match="every"):
        run.set_rdf(PAIRS, every=0)
    run.step()
    assert run.rdf()["frames"] == 3
    ani.close()
