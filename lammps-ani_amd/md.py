"""A LAMMPS-free stand-in for the timestep loop that drives ``PairANI::compute`` in the reference's runs.

The reference is always run under LAMMPS' velocity-Verlet integrator (``run N`` with ``fix nve`` [+ ``fix langevin``],
``neighbor 2.0 bin``, ``neigh_modify every 10 delay 0 check yes`` — examples/benchmark/in.lammps:24-26,54-72); its
headline ns/day is the rate of THAT loop.  ``VerletRun`` reproduces the loop's order of operations around the C ABI with
everything resident on the GPU:

    initial_integrate -> [displacement check every `every` steps -> device neighbour list (ani_build_list_device)]
    -> forward ghost positions -> force_clear -> ani_compute_full_device -> reverse ghost forces -> post_force fixes
    -> final_integrate

Only device memory, streams and torch.distributed come from torch; the arithmetic of the hot path is libani_hip's.

Re-neighbouring (LAMMPS: Domain::pbc + Comm::exchange + Comm::borders + Neighbor::build) is done on the device as
well, by ``comm.DomainComm``: owned atoms are wrapped into the box and handed to the rank whose brick now holds them,
the ghost shell (periodic images included) is rebuilt from the current positions, then the library builds the full
list (ani_build_list_device).  One rank or several, the run can go on indefinitely; between rebuilds only the ghost
positions (forward) and ghost forces (reverse) travel, one message per peer and direction.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.distributed as dist

from .ani_hip import NPT_LAYOUT, SHAKE_STATS_KEYS

# LAMMPS `units real` constants (update.cpp of LAMMPS): forces kcal/mol/A, masses g/mol, time fs
FTM2V = 1.0 / 48.88821291 / 48.88821291
MVV2E = 48.88821291 * 48.88821291
BOLTZ = 0.0019872067

# g/mol by ANI-2x species order H C N O S F Cl (the reference's data files carry the same values in `Masses`)
ANI2X_MASSES = (1.008, 12.011, 14.007, 15.999, 32.06, 18.998, 35.45)


def constraint_clusters(bonds, tags):
    """The clusters of ``VerletRun.set_constraints`` (LAMMPS FixShake::find_clusters, without its angle form): every connected
    component of the constrained bonds has to be a star -- one centre bonded to one, two or three partners that have no other
    constrained bond.  bonds: [nb, 2] global tags; tags: [nlocal], the global tag of every local index.
    Returns (cl [nc, 4] int32: centre and partners as local indices, -1 in unused slots; slot_bond [nc, 3] int64: which row of
    `bonds` slot k is, -1 unused), clusters ordered by size, then by centre index, the partners of a centre ascending.  A
    two-atom component takes its lower local index as the centre.  Raises ValueError naming the offending tag for an unknown
    tag, a self-bond, a duplicate bond, a component that is not a star and a centre with more than three partners."""
    bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    tags = np.asarray(tags, dtype=np.int64).reshape(-1)
    local = {int(t): i for i, t in enumerate(tags.tolist())}
    seen, nbrs = set(), {}
    for b, (ta, tb) in enumerate(bonds.tolist()):
        for t in (ta, tb):
            if t not in local:
                raise ValueError(f"constraint bond {b} ({ta}, {tb}): unknown tag {t}")
        if ta == tb:
            raise ValueError(f"constraint bond {b}: self-bond on tag {ta}")
        key = (min(ta, tb), max(ta, tb))
        if key in seen:
            raise ValueError(f"constraint bond {b}: duplicate of the bond between tags {key[0]} and {key[1]}")
        seen.add(key)
        nbrs.setdefault(local[ta], []).append((local[tb], b))
        nbrs.setdefault(local[tb], []).append((local[ta], b))
    found = []
    for i, nb in nbrs.items():
        if len(nb) == 1:
            j, b = nb[0]
            if len(nbrs[j]) == 1 and i < j:
                found.append((i, nb))
            continue
        for j, _ in nb:
            if len(nbrs[j]) > 1:
                raise ValueError(f"constraint clusters: the component of tag {int(tags[i])} is not a star (tag {int(tags[i])} and its "
                                 f"partner tag {int(tags[j])} both have further constrained bonds)")
        if len(nb) > 3:
            raise ValueError(f"constraint clusters: tag {int(tags[i])} is the centre of {len(nb)} constrained bonds (at most 3)")
        found.append((i, sorted(nb)))
    found.sort(key=lambda c: (len(c[1]), c[0]))
    cl = np.full((len(found), 4), -1, dtype=np.int32)
    slot_bond = np.full((len(found), 3), -1, dtype=np.int64)
    for c, (i, nb) in enumerate(found):
        cl[c, 0] = i
        for k, (j, b) in enumerate(nb):
            cl[c, 1 + k], slot_bond[c, k] = j, b
    return cl, slot_bond


def npt_rebuild_limit(skin, lo_built, len_built, lo_now, len_now, nimg_max) -> float:
    """The squared displacement of an owned atom since the build above which a loop whose box moves re-neighbours:
    max(0, (skin - nimg_max (d_lo + d_hi)) / 2)^2, with d_lo and d_hi the Euclidean displacements of the two box corners since the
    build and nimg_max the largest image count of the ghost shell.  A pair's distance changes by at most the two owners'
    displacements plus the change of the image shift between them; the displacements are taken against the unscaled positions of
    the build, so they include the dilation, and a shift of up to nimg_max box lengths changes by at most nimg_max (d_lo + d_hi).
    With one image this is Neighbor::check_distance with `boxcheck`; with a box at rest it is the constant (skin / 2)^2."""
    lo_b, len_b, lo_n, len_n = (np.asarray(a, dtype=np.float64) for a in (lo_built, len_built, lo_now, len_now))
    d_lo = float(np.sqrt(((lo_n - lo_b) ** 2).sum()))
    d_hi = float(np.sqrt(((lo_n + len_n - lo_b - len_b) ** 2).sum()))
    return max(0.0, 0.5 * (skin - nimg_max * (d_lo + d_hi))) ** 2


class VerletRun:
    def __init__(self, ani, inp, box_len, device, dt: float = 0.5, cutoff: float = 5.1, skin: float = 2.0,
                 every: int = 10, masses=ANI2X_MASSES, group=None, seed: int = 12345,
                 langevin=None, box_lo=None, grid=None, periodic=(True, True, True), overlap=None, native_comm=None,
                 force_collectives=False, vflag=False, atom_masses=None):
        """ani: ani_hip.ANI (full list, any precision); inp: harness.RankInput of this rank — only its OWNED atoms
        (positions, types, global tags) are taken, ghosts and lists are rebuilt here; langevin: None or
        (T_target, damp_fs) as ``fix langevin T T damp seed``; grid: processor grid (default comm.grid_for(world));
        overlap: run the two ghost
        exchanges of a step on a second stream beside the rows that do not need them (the library's split step,
        include/ani_hip.h ani_step_*).  Cutting the step costs five more launches (+0.05 ms at 12 500 atoms per GPU,
        measured on one card), which the hidden exchanges have to pay back: default on with several ranks over RCCL (two
        latency-bound all-to-alls per step), off otherwise; environment ANI_MD_OVERLAP=0/1 overrides the default.
        native_comm: an ani_hip.NativeComm -- the exchanges then run inside libani_hip.so as grouped ncclSend / ncclRecv
        (include/ani_comm.h) instead of torch.distributed collectives; force_collectives: a single rank takes the several-rank
        paths (one-participant collectives), so that one GPU can exercise them.  vflag: every force evaluation also
        accumulates the pair style's virial (``virial()``; LAMMPS sets vflag on thermo steps with a pressure compute).
        atom_masses: [nlocal] g/mol in the order of inp's owned atoms (``fix property/atom rmass``, hydrogen mass repartitioning):
        they take the place of the lookup by species wherever the loop uses a mass.  One rank with native re-neighbouring only (the
        owned atoms keep their order there)."""
        if torch.device(device).type != "cuda":
            raise ValueError(f"VerletRun needs a HIP device (torch device type 'cuda'), got {device!r}: every step of the loop is one of "
                             "libani_hip's device entry points (include/ani_md.h, ani_build_list_device), which take device pointers")
        from . import ani_hip
        from .comm import DomainComm, grid_for
        self.ani, self.device, self.group = ani, device, group
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.dt, self.cutneigh, self.skin, self.every = float(dt), cutoff + skin, skin, int(every)
        self._d2_rebuild = (0.5 * skin) ** 2   # Neighbor::check_distance: rebuild once an atom has moved more than skin/2
        box_lo = np.zeros(3) if box_lo is None else np.asarray(box_lo, dtype=np.float64)
        self._box_lo_np = box_lo
        self._box_len_np = np.asarray(box_len, dtype=np.float64)
        self.dc = DomainComm(grid or grid_for(world), box_lo, box_len, self.cutneigh, device, group=group, periodic=periodic,
                             native=native_comm, force_collectives=force_collectives)
        self.native = native_comm
        self.vflag = bool(vflag)
        self.masses = torch.as_tensor(np.asarray(masses, dtype=np.float64), device=device)
        self.langevin = langevin
        n = inp.nlocal
        self._atom_masses = None
        if atom_masses is not None:
            am = np.asarray(atom_masses, dtype=np.float64).reshape(-1)
            if am.shape[0] != n or not (np.isfinite(am).all() and (am > 0.0).all()):
                raise ValueError(f"VerletRun: atom_masses must be {n} positive finite masses (one per owned atom), got {am.shape[0]}")
            if self.dc.multi:
                raise RuntimeError("VerletRun: atom_masses: one rank only (the masses would have to migrate with their atoms)")
            self._atom_masses = torch.as_tensor(am, device=device).contiguous()
        self.nlocal = n
        self.x = torch.as_tensor(inp.x[:n], dtype=torch.float64, device=device).contiguous()
        self.species = torch.as_tensor(inp.species[:n].astype(np.int32), device=device)
        self.tag = torch.as_tensor(np.asarray(inp.tag[:n]).astype(np.int64), device=device)
        self.v = torch.zeros((n, 3), dtype=torch.float64, device=device)
        self.ev = torch.zeros(10, dtype=torch.float64, device=device)
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(seed + 7919 * (dist.get_rank(group) if dist.is_initialized() else 0))
        self.step_no = 0
        self.since_build = 0
        self.nbuilds = 0
        self.npairs = 0
        self._stream = torch.cuda.current_stream(device).cuda_stream
        self._seed = int(seed)
        # the loop's own steps (fix nve, fix langevin, displacement check, one-rank ghost copies) are the kernels of include/ani_md.h
        self._md = ani_hip.lib()
        self._d2max = torch.zeros(1, dtype=torch.float64, device=device)
        self._sendbuf = torch.empty((0, 3), dtype=torch.float64, device=device)
        self._recvbuf = torch.empty((0, 3), dtype=torch.float64, device=device)
        ani.set_option("device_overwrite_forces", 1)   # no separate force_clear launch
        env = os.environ.get("ANI_MD_OVERLAP")
        # default off: cutting the step costs +0.05 ms on one card and its benefit has not been measured on several
        want = False if overlap is None else bool(overlap)
        if env is not None and overlap is None:
            want = env not in ("", "0")
        self._overlap = bool(want)
        self._want_fold = os.environ.get("ANI_MD_FOLD", "1") not in ("", "0")   # measurement knob: 0 keeps the two ghost kernels
        self._fold = False
        # one rank: re-neighbouring (position wrap, ghost shell, buffers, displacement check) through the kernels of
        # include/ani_md.h instead of tensor operations; ANI_MD_NATIVE_REBUILD=0 keeps the tensor forms (measurements, tests)
        self._native_rebuild = bool(not self.dc.multi and os.environ.get("ANI_MD_NATIVE_REBUILD", "1") not in ("", "0"))
        if self._atom_masses is not None and not self._native_rebuild:
            raise RuntimeError("VerletRun: atom_masses needs the device loop with native re-neighbouring (one rank on the GPU)")
        self._cap = 0
        self._cons = None      # bond constraints (set_constraints): None, or the device tables and parameters of the two stages
        self._ncons = 0        # constrained bonds: degrees of freedom that temperature() does not count
        self._rdf_every = 0    # radial distribution functions (set_rdf): 0 = none, else a frame every so many steps
        self._nvt = None       # Nose-Hoover chain (set_nvt): None, or the device record, scratch and parameters
        self._npt = None       # isotropic barostat (set_npt): None, or the device record, its check buffers, parameters and targets
        self._restr = None     # umbrella restraints (set_restraints): None, or the device tables, outputs, record and series
        self._img = None       # image flags (set_images): None, or the [nlocal, 3] int32 table that the wrap keeps
        self._msd = None       # mean-squared displacements (set_msd): None, or the classes, the origin, scratch, outputs and series
        self._dump = None      # trajectory frames (set_dump): None, or the device ring, its host side and the DCD writer
        self._com = None       # centre-of-mass record, scratch and host words (com_state, zero_momentum, ...), made at first use
        self._mom = None       # fix momentum (set_momentum): None, or every and the flags of ani_md_com_apply
        self._recenter = None  # fix recenter (set_recenter): None, or the fractions and the dimension mask
        self._tag_order = None  # the owned atoms in ascending order of their global tag (_tag_rank), made at first use
        self._thermo_buf = None
        if self._overlap:
            # ANI_MD_OVERLAP_ONE_STREAM: measurement knob, the same cut step with everything on the compute stream
            self._comm_stream = torch.cuda.current_stream(device) if os.environ.get("ANI_MD_OVERLAP_ONE_STREAM") else \
                torch.cuda.Stream(device=device)
            self._ev = [torch.cuda.Event() for _ in range(4)]
        self._build_list()
        self._forces()
        self._post_force()

    # ---- pieces of the loop ---------------------------------------------------------------------------
    def _allreduce(self, t: torch.Tensor, op: str) -> torch.Tensor:
        """t reduced over the ranks (op: "sum" or "max"), in place where it can be: inside libani_hip.so with a native
        communicator, through a host copy under gloo (which takes no device tensor), torch.distributed otherwise.  With one
        participant (one rank, or force_collectives) every form leaves the values as they are."""
        if self.native is not None and self.dc.multi and t.is_cuda and t.dtype == torch.float64:
            self.native.allreduce(t.data_ptr(), t.numel(), op, stream=self._stream)
        elif dist.is_initialized() and (dist.get_world_size(self.group) > 1 or self.dc.multi):
            if dist.get_backend(self.group) == "gloo" and t.is_cuda:
                t = t.cpu()
            dist.all_reduce(t, op=dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM, group=self.group)
        return t

    def _allreduce_max(self, t: torch.Tensor) -> float:
        return float(self._allreduce(t, "max"))

    def _allreduce_sum(self, t: torch.Tensor) -> float:
        return float(self._allreduce(t, "sum"))

    def _per_atom_factors(self):
        """mass-dependent factors of the integrator, expanded once per re-neighbouring (atoms may have migrated) so
        that each update is ONE device kernel"""
        n = self.nlocal
        if not self.dc.multi and getattr(self, "_factors_n", -1) == n:
            return   # one rank: nobody migrates, the owned atoms keep their order
        self._factors_n = n
        am = getattr(self, "_atom_masses", None)
        m = self.masses[self.species[:n].long()] if am is None else am
        self.mass = m[:, None]
        self._dtfm1 = (0.5 * self.dt * FTM2V) / m                        # [n], the kernels' form
        self._g1 = self._g2 = None
        if self.langevin is not None:
            T, damp = self.langevin
            self._g1 = m * (-1.0 / damp / FTM2V)
            self._g2 = torch.sqrt(m) * ((24.0 * BOLTZ * T / damp / self.dt / MVV2E) ** 0.5 / FTM2V)

    def _grow(self, ntotal: int):
        """capacity buffers of the per-atom arrays that include ghosts (grown 1.5x, owned rows kept)"""
        if ntotal <= self._cap:
            return
        cap = ntotal + ntotal // 2 + 64
        n = self.nlocal
        xb = torch.empty((cap, 3), dtype=torch.float64, device=self.device)
        sb = torch.empty(cap, dtype=torch.int32, device=self.device)
        xb[:n].copy_(self.x[:n])
        sb[:n].copy_(self.species[:n])
        self._xbuf, self._spbuf = xb, sb
        self._fbuf = torch.zeros((cap, 3), dtype=torch.float64, device=self.device)
        self._sidx = torch.empty(cap, dtype=torch.int64, device=self.device)
        self._sshift = torch.empty((cap, 3), dtype=torch.float64, device=self.device)
        self._cap = cap

    def _build_list_native(self):
        """Domain::pbc + Comm::borders + Neighbor::build of a one-rank run without tensor operations: wrap kernel, ghost shell by
        count / scan / fill (one host read of the ghost count), ghosts appended in place, device list, ghost fold."""
        n, dc, md, st = self.nlocal, self.dc, self._md, self._stream
        if self._cap == 0:
            self._grow(max(self.x.shape[0], n))
            self._xbuilt_buf = torch.empty((n, 3), dtype=torch.float64, device=self.device)
            self._chk_dev = torch.zeros(1, dtype=torch.float64, device=self.device)
            self._chk_host = torch.zeros(1, dtype=torch.float64).pin_memory()
            self._ncombo = -1
            self._shell_tables()
            self._lo3 = np.array(self._box_lo_np, dtype=np.float64)
            self._len3 = np.array(self._box_len_np, dtype=np.float64)
            self._pmask = sum(1 << k for k in range(3) if dc.periodic[k])
        if self._npt is not None and not self._npt["fresh"]:
            self._npt_read_box()      # a rebuild that no look of the host precedes: one read of the record
        x = self._xbuf
        if self._img is None:
            self._check(md.ani_md_wrap_positions(x.data_ptr(), n, self._lo3.ctypes.data, self._len3.ctypes.data, self._pmask, st))
        else:     # the same wrap, which adds the box lengths it removes to the image flags
            self._check(md.ani_md_wrap_positions_images(x.data_ptr(), self._img.data_ptr(), n, self._lo3.ctypes.data,
                                                        self._len3.ctypes.data, self._pmask, st))
        ng = 0
        nblk = max((n + 255) // 256, 1)
        half = max(self._ncombo, 1) * nblk
        if self._ncombo:
            self._check(md.ani_md_ghost_shell_count(x.data_ptr(), n, self._clo2.data_ptr(), self._chi2.data_ptr(), self._ncombo,
                                                    self._blk.data_ptr(), self._blk[half:].data_ptr(), self._cnt_dev.data_ptr(), st))
            self._cnt_host.copy_(self._cnt_dev, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()      # the ghost count sizes the buffers (rebuild steps only)
            ng = int(self._cnt_host[0])
        if n + ng > self._cap:
            self.x, self.species = self._xbuf[:n], self._spbuf[:n]
            self._grow(n + ng)
            x = self._xbuf
        if ng:
            self._check(md.ani_md_ghost_shell_fill(x.data_ptr(), n, self._clo2.data_ptr(), self._chi2.data_ptr(), self._cshift2.data_ptr(),
                                                   self._ncombo, self._blk[half:].data_ptr(), self._sidx.data_ptr(),
                                                   self._sshift.data_ptr(), st))
            self._check(md.ani_md_append_ghosts(x.data_ptr(), self._spbuf.data_ptr(), n, self._sidx.data_ptr(), self._sshift.data_ptr(), ng, st))
        dc.send_idx, dc.send_shift = self._sidx[:ng], self._sshift[:ng]
        dc.send_splits, dc.recv_splits, dc.nlocal, dc.nghost = [ng], [ng], n, ng
        self.ntotal = n + ng
        self.x, self.species, self.f = self._xbuf[: self.ntotal], self._spbuf[: self.ntotal], self._fbuf[: self.ntotal]
        self._per_atom_factors()
        lo = dc.sub_lo - self.cutneigh - 0.25
        hi = dc.sub_hi + self.cutneigh + 0.25
        # the fold goes in with the list: its check rides on the build's own synchronisation
        self._fold = bool(self._want_fold and self.ani.use_single and not self._overlap)
        if self._fold:
            self.ani.stage_ghost_fold(dc.send_idx.data_ptr(), dc.send_shift.data_ptr(), ng)
        self.npairs = self.ani.build_list_device(self.ntotal, n, self.species.data_ptr(), self.x.data_ptr(), self.cutneigh, lo, hi, stream=st)
        self._xbuilt_buf.copy_(self.x[:n])
        self.x_built = self._xbuilt_buf
        self._check(md.ani_md_check(self._d2max.data_ptr(), self.ev.data_ptr(), self._chk_dev.data_ptr(), st))   # zeroes the maximum
        if self._npt is not None:     # the box this list belongs to: what the re-neighbouring limit measures from
            self._npt.update(lo_built=self._box_lo_np.copy(), len_built=self._box_len_np.copy(), nimg_max=dc.nimg_max)
        self.since_build = 0
        self.nbuilds += 1

    def _shell_tables(self):
        """the ghost shell's combination table of the DomainComm as the [ncombo, 3] arrays of the shell kernels, and their count
        buffers: made at the first build, and again whenever the box has changed (the number of combinations can change with it)"""
        dc, n = self.dc, self.nlocal
        self._clo2 = dc._clo.reshape(-1, 3).contiguous()
        self._chi2 = dc._chi.reshape(-1, 3).contiguous()
        self._cshift2 = dc._shift.reshape(-1, 3).contiguous()
        ncombo = int(self._clo2.shape[0])
        if ncombo != self._ncombo:
            self._ncombo = ncombo
            nblk = max((n + 255) // 256, 1)
            self._blk = torch.empty(2 * max(ncombo, 1) * nblk, dtype=torch.int32, device=self.device)
            self._cnt_dev = torch.zeros(ncombo + 1, dtype=torch.int32, device=self.device)
            self._cnt_host = torch.zeros(ncombo + 1, dtype=torch.int32).pin_memory()

    def _set_box(self, lo, length):
        """The host's copy of a box that the device has moved: the loop's own arrays, the DomainComm geometry with its combination
        table, and the shell kernels' tables.  Raises for a box that is not finite or not positive."""
        lo, length = np.array(lo, dtype=np.float64), np.array(length, dtype=np.float64)
        if not (np.isfinite(lo).all() and np.isfinite(length).all() and (length > 0.0).all()):
            raise RuntimeError(f"the barostat's box is not finite or not positive: lo {lo.tolist()}, len {length.tolist()}")
        if (lo == self._box_lo_np).all() and (length == self._box_len_np).all():
            return
        self._box_lo_np, self._box_len_np = lo, length
        self._lo3[:], self._len3[:] = lo, length
        self.dc.set_box(lo, length)
        self._shell_tables()

    def _build_list(self):
        """Domain::pbc + Comm::exchange + Comm::borders + Neighbor::build."""
        if self._native_rebuild:
            return self._build_list_native()
        n = self.nlocal
        xo, v, tag, sp = self.dc.exchange(self.x[:n], self.v, self.tag, self.species[:n])
        self.nlocal = n = xo.shape[0]
        self.v, self.tag = v.contiguous(), tag.contiguous()
        self.x, self.species = self.dc.borders(xo, sp.contiguous())
        self.ntotal = self.x.shape[0]
        self._per_atom_factors()
        self.f = torch.zeros((self.ntotal, 3), dtype=torch.float64, device=self.device)
        # every atom lies inside the rank's brick widened by the ghost cutoff
        lo = self.dc.sub_lo - self.cutneigh - 0.25
        hi = self.dc.sub_hi + self.cutneigh + 0.25
        self.npairs = self.ani.build_list_device(self.ntotal, n, self.species.data_ptr(), self.x.data_ptr(),
                                                 self.cutneigh, lo, hi, stream=self._stream)
        # one rank: every ghost is an image of an owned atom -- the library's first and last kernel of a step do the two ghost
        # exchanges themselves (ani_set_ghost_fold); the maps belong to this list
        self._fold = False
        if self._want_fold and not self.dc.multi and self.ani.use_single and not self._overlap:
            self.ani.set_ghost_fold(self.dc.send_idx.data_ptr(), self.dc.send_shift.data_ptr(), self.ntotal - n, stream=self._stream)
            self._fold = True
        self.x_built = self.x[:n].clone()
        self._d2max.zero_()
        self.since_build = 0
        self.nbuilds += 1

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"ani_md kernel launch failed (hipError {rc})")

    def _forces(self):
        """PairANI::compute (which overwrites f: no force_clear) + reverse communication of the ghost forces"""
        self.ani.compute_device(self.ntotal, self.nlocal, None, self.x.data_ptr(), self.npairs, None, None, None, 1,
                                self.f.data_ptr(), self.ev.data_ptr(), vflag=self.vflag, stream=self._stream)
        if not self._fold:   # folded: the finish kernel has added the images' rows into their owners'
            self._reverse_ghosts()

    def _post_force(self):
        """fix langevin (LAMMPS fix_langevin.cpp, uniform random numbers in [-0.5, 0.5)): f += g1 v + g2 r on owned atoms.
        Tensor-operation form from the [n] factors: it runs once, at set-up (a step has it inside ani_md_final_integrate)."""
        if self._g1 is not None:
            g1, g2 = self._g1[:, None], self._g2[:, None]
            r = torch.empty((self.nlocal, 3), dtype=torch.float64, device=self.device)
            r.uniform_(-0.5, 0.5, generator=self.gen)
            fl = self.f[: self.nlocal]
            fl.addcmul_(g1, self.v)
            fl.addcmul_(g2, r)

    def create_velocities(self, T: float, rot: bool = False):
        """``velocity all create T seed mom yes dist gaussian`` (examples/benchmark/in.lammps:54).  rot: ``rot yes`` as well -- the
        angular momentum about the centre of mass is taken out (zero_momentum) before the rescale."""
        if rot:
            self._protocol_guard("create_velocities(rot=True)")
            self._need_images("create_velocities(rot=True)")
        if T <= 0.0:
            self.v.zero_()
            return
        sigma = torch.sqrt(BOLTZ * T / (self.mass * MVV2E))
        self.v = sigma * torch.randn((self.nlocal, 3), dtype=torch.float64, device=self.device, generator=self.gen)
        p = (self.mass * self.v).sum(0)
        mtot = self.mass.sum().reshape(1)
        if dist.is_initialized() and dist.get_world_size(self.group) > 1:
            pm = torch.cat([p, mtot])
            pm = pm.cpu() if dist.get_backend(self.group) == "gloo" else pm
            dist.all_reduce(pm, group=self.group)
            pm = pm.to(self.device)
            p, mtot = pm[:3], pm[3:]
        self.v -= p / mtot
        if rot:
            self.zero_momentum(linear=False, angular=True)
        if self._cons is not None:
            self.project_velocities()   # the components along the constrained bonds carry no temperature: out before the rescale
        ke = self.kinetic_energy()
        n = self._allreduce_sum(torch.tensor([float(self.nlocal)], dtype=torch.float64, device=self.device))
        t_now = 2.0 * ke / (3.0 * n - 3.0 - self._ncons) / BOLTZ
        self.v *= (T / t_now) ** 0.5

    # ---- the schedule of a step: first half, middle, second half ---------------------------------------
    def _first_half(self, t_target=None, npart: int = 0, p_target=None):
        """fix nve / fix nvt initial_integrate: v += dtf f / m ; x += dt v  (+ the displacement maximum of check_distance),
        behind the chain's half-step with a thermostat (v = s v first); with a barostat the chains' half-step that also moves the box
        in its record, then the dilated move of the atoms and the scaling of the ghost shifts in one launch; then the position
        stage of the constraints"""
        nvt = self._nvt
        if self._npt is not None:
            self._npt_chain(0, t_target, p_target, npart)
            self._npt["fresh"] = False     # the box moves: the host's copy is behind until it looks
            self._check(self._md.ani_md_npt_initial_integrate(self.x.data_ptr(), self.v.data_ptr(), self.f.data_ptr(),
                                                              self._dtfm1.data_ptr(), self.dt, self.nlocal, self.x_built.data_ptr(),
                                                              self._d2max.data_ptr(), nvt["state"].data_ptr(),
                                                              self._npt["state"].data_ptr(), self._sshift.data_ptr(),
                                                              self.ntotal - self.nlocal, self._stream))
        elif nvt is not None:
            self._nvt_chain(t_target, npart)
            self._check(self._md.ani_md_nh_initial_integrate(self.x.data_ptr(), self.v.data_ptr(), self.f.data_ptr(),
                                                             self._dtfm1.data_ptr(), self.dt, self.nlocal, self.x_built.data_ptr(),
                                                             self._d2max.data_ptr(), nvt["state"].data_ptr(), self._stream))
        else:
            self._check(self._md.ani_md_initial_integrate(self.x.data_ptr(), self.v.data_ptr(), self.f.data_ptr(),
                                                          self._dtfm1.data_ptr(), self.dt, self.nlocal, self.x_built.data_ptr(),
                                                          self._d2max.data_ptr(), self._stream))
        if self._cons is not None:
            self._shake_positions()
        if self._recenter is not None:
            self._recenter_now()

    def _middle(self, force_rebuild: bool = False):
        """between the two integrator halves: re-neighbouring decision, ghost positions, forces, ghost forces"""
        self.step_no += 1
        self.since_build += 1
        # Neighbor::decide + check_distance (every N steps, rebuild if any atom moved more than skin/2)
        rebuild = bool(force_rebuild) or (self.since_build % self.every == 0 and self._look() > self._rebuild_limit())
        self._ghosts_and_forces(rebuild, sample=True)
        # on every path above the ghost rows of x are now the images of this step's owned positions
        if self._rdf_every and self.step_no % self._rdf_every == 0:
            self.ani.rdf_accumulate_device(self.ntotal, self.nlocal, self.x.data_ptr(), stream=self._stream)
        msd, dump = self._msd, self._dump
        if msd is not None and msd["stride"] and self.step_no % msd["stride"] == 0:
            row = msd["series"][msd["nsamples"] % msd["capacity"]].data_ptr()
            msd["nsamples"] += 1
            self._msd_sample(row)
        if dump is not None and self.step_no % dump["every"] == 0:
            self._dump_frame()

    def _rebuild_limit(self) -> float:
        """what the worst squared displacement of a look is held against: (skin / 2)^2, or npt_rebuild_limit with the box of the
        look (which has just refreshed the host's copy) against the box of the build"""
        npt = self._npt
        if npt is None:
            return self._d2_rebuild
        return npt_rebuild_limit(self.skin, npt["lo_built"], npt["len_built"], self._box_lo_np, self._box_len_np, npt["nimg_max"])

    def _second_half(self, t_target=None, p_target=None):
        """fix langevin post_force + fix nve final_integrate and the velocity stage of the constraints; with a thermostat the
        pass that also leaves the partial sums of sum m v^2 (constrained: the plain one, the velocity stage, then the sums), the
        chain's half-step on them and the scaling (a uniform scale keeps r . (v_c - v_p) = 0)"""
        nvt = self._nvt
        if self._npt is not None:
            self._check(self._md.ani_md_npt_final_integrate(self.v.data_ptr(), self.f.data_ptr(), self._dtfm1.data_ptr(),
                                                            nvt["mass"].data_ptr(), self.nlocal, self._npt["state"].data_ptr(),
                                                            nvt["work"].data_ptr(), self._stream))
            self._npt_chain(1, t_target, p_target, nvt["npart"])
            self._check(self._md.ani_md_nh_scale(self.v.data_ptr(), self.nlocal, nvt["state"].data_ptr(), self._stream))
            return
        if nvt is None or self._cons is not None:
            self._final_integrate()
            self.project_velocities()
            if nvt is not None:
                self._nvt_kinetic()
        else:
            self._check(self._md.ani_md_nh_final_integrate(self.v.data_ptr(), self.f.data_ptr(), self._dtfm1.data_ptr(),
                                                           nvt["mass"].data_ptr(), self.nlocal, nvt["work"].data_ptr(), self._stream))
        if nvt is not None:
            self._nvt_chain(t_target, nvt["npart"])
            self._check(self._md.ani_md_nh_scale(self.v.data_ptr(), self.nlocal, nvt["state"].data_ptr(), self._stream))

    def _steps(self, nsteps: int, t_from=None, t_to=None, force_rebuild: bool = False, before_forces=None, after_forces=None,
               p_from=None, p_to=None):
        """nsteps steps of first half, middle, second half; with a thermostat the target goes from t_from (exclusive) to t_to (at
        the last step), and the call begins with the sum of the velocities as they are.  The one exception to the three pieces:
        where nothing stands between the second half of a step and the first half of the next -- no thermostat, no constraints, no
        fix momentum on that step -- the two are ONE launch, which carries the number of the step that ends."""
        nvt, mom = self._nvt, self._mom
        one_launch = nvt is None and self._cons is None
        t = p = None
        if nvt is not None:
            self._nvt_kinetic()
        fresh = nvt is not None      # the chain's next half-step sums the scratch; otherwise it goes on from the sum it scaled itself
        moved = False                # the first half of this step ran in the launch that ended the last one
        for k in range(nsteps):
            if nvt is not None:
                t = t_to if k + 1 == nsteps else t_from + ((k + 1) / nsteps) * (t_to - t_from)
            if p_to is not None:
                p = p_to if k + 1 == nsteps else p_from + ((k + 1) / nsteps) * (p_to - p_from)
            if not moved:
                self._first_half(t, nvt["npart"] if fresh else 0, p)
                fresh = False
            if before_forces is not None:
                before_forces(k)
            self._middle(force_rebuild)
            if after_forces is not None:
                after_forces(k)
            mom_now = mom is not None and self.step_no % mom["every"] == 0
            moved = one_launch and k + 1 < nsteps and not mom_now
            if moved:
                lgv = self._g1 is not None
                self._check(self._md.ani_md_final_initial_integrate(
                    self.x.data_ptr(), self.v.data_ptr(), self.f.data_ptr(), self._dtfm1.data_ptr(), self.dt, self.nlocal,
                    1 if lgv else 0, self._g1.data_ptr() if lgv else None, self._g2.data_ptr() if lgv else None,
                    self.tag.data_ptr(), self._seed, self.step_no, self.x_built.data_ptr(), self._d2max.data_ptr(), self._stream))
            else:
                self._second_half(t, p)
            if moved and self._recenter is not None:
                self._recenter_now()         # behind the first half that the launch above held
            if mom_now:                      # fix momentum end_of_step: on the full-step velocities
                self._com_sample()
                self._com_apply(mom["flags"])
                if nvt is not None:          # the chain goes on from the sum of the velocities as they are now
                    self._nvt_kinetic()
                    fresh = True

    def step(self, force_rebuild: bool = False):
        """force_rebuild: re-neighbour in this step whatever the displacement check would say (measurements).  With a thermostat
        (set_nvt) the step begins with a fresh kinetic sum and uses the current target: N calls agree with run(N) to the rounding of
        that sum, not bitwise."""
        t = self._nvt["t_target"] if self._nvt is not None else None
        p = self._npt["p_target"] if self._npt is not None else None
        self._steps(1, t, t, force_rebuild, p_from=p, p_to=p)

    def run(self, nsteps: int, before_forces=None, after_forces=None):
        """``run N`` without per-step output: nothing looks at the full-step velocities between two steps, so the
        final_integrate of a step and the initial_integrate of the next are ONE kernel (same arithmetic and rounding as
        step() N times; the loop is in a full-step state again when this returns).  before_forces(k) / after_forces(k):
        optional callables around the force evaluation of step k (the bench's phase-timer switches).  With a thermostat (set_nvt)
        or constraints the halves are the separate launches of step(); the thermostat's target ramps from t_start to t_stop over
        the nsteps."""
        if nsteps <= 0:
            return
        nvt, npt = self._nvt, self._npt
        if nvt is None:
            self._steps(int(nsteps), None, None, False, before_forces, after_forces)
        elif npt is not None:
            self._steps(int(nsteps), nvt["t_start"], nvt["t_stop"], False, before_forces, after_forces, npt["p_start"], npt["p_stop"])
            nvt["t_target"], npt["p_target"] = nvt["t_stop"], npt["p_stop"]
        else:
            self._steps(int(nsteps), nvt["t_start"], nvt["t_stop"], False, before_forces, after_forces)
            nvt["t_target"] = nvt["t_stop"]

    # ---- the host's look at the device ---------------------------------------------------------------------------------
    def _look(self, extra=None, word=None) -> float:
        """The worst squared displacement of an owned atom since the last look, which this zeroes; raises when the last energy is
        not finite -- the device entry point cannot return ANI_ERR_CAPACITY (nothing synchronises), it turns the energy into NaN
        instead, and this host round trip carries that along -- and, with constraints, when a cluster solve did not converge (the
        stats words sit behind the maximum: the same read).  With native re-neighbouring one kernel and one pinned read;
        otherwise a copy of the word and an all-reduce over the ranks.  extra: (state, device words, pinned words) of minimize(),
        whose check kernel puts the FIRE record behind the maximum; minimize() judges the two together, with on_look in between.
        word: a scratch word in place of the loop's own maximum (warm_paths: nothing is zeroed that the loop needs, nothing is
        judged)."""
        d2max = self._d2max if word is None else word
        npt = self._npt if (extra is None and word is None) else None
        if self._native_rebuild:
            if npt is not None:   # the barostat record behind the word: the same read brings the box of this moment
                dev, host = npt["chk_dev"], npt["chk_host"]
                self._check(self._md.ani_md_npt_check(d2max.data_ptr(), self.ev.data_ptr(), npt["state"].data_ptr(), dev.data_ptr(), self._stream))
            elif extra is None:
                dev, host = self._chk_dev, self._chk_host
                self._check(self._md.ani_md_check(d2max.data_ptr(), self.ev.data_ptr(), dev.data_ptr(), self._stream))
            else:
                state, dev, host = extra
                self._check(self._md.ani_md_fire_check(d2max.data_ptr(), self.ev.data_ptr(), state.data_ptr(), dev.data_ptr(), self._stream))
            host.copy_(dev, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            worst = float(host[0])    # the running maximum, or +inf when the last energy is not finite
        else:
            d2 = d2max.clone()    # running maximum since the last look (monotone between rebuilds: same decision)
            d2max.zero_()
            d2 = torch.where(torch.isfinite(self.ev[:1]), d2, torch.full_like(d2, float("inf")))
            worst = self._allreduce_max(d2.clone())
        if extra is not None or word is not None:
            return worst
        if worst == float("inf"):
            raise RuntimeError("non-finite energy from the device step: a neighbour count exceeded the kernels' LDS "
                               "capacity (ANI_ERR_CAPACITY) or the forces diverged")
        if npt is not None:
            rec = npt["chk_host"][1:].numpy()
            self._set_box(rec[NPT_LAYOUT["lo"]], rec[NPT_LAYOUT["len"]])
            npt["fresh"] = True
        if self._cons is not None and self._native_rebuild:
            self._constraint_health(self._chk_host[1:])
        return worst

    # ---- ghost exchanges ------------------------------------------------------------------------------------------------
    def _msgbuf(self, name: str, rows: int) -> torch.Tensor:
        """the send or receive buffer of the all-to-all exchanges (name: _sendbuf / _recvbuf), made anew when the count changed"""
        buf = getattr(self, name)
        if buf.shape[0] != rows:
            buf = torch.empty((rows, 3), dtype=torch.float64, device=self.device)
            setattr(self, name, buf)
        return buf

    def _forward_ghosts(self, stream):
        """forward exchange: x[nlocal:] <- the owners' positions (+ image shifts); kernels and native messages on `stream`, the
        all-to-all on torch's current stream"""
        dc = self.dc
        if not dc.multi:
            self._check(self._md.ani_md_forward_ghosts(self.x.data_ptr(), dc.send_idx.data_ptr(), dc.send_shift.data_ptr(),
                                                       self.nlocal, self.ntotal - self.nlocal, stream))
        elif self.native is not None:
            self.native.forward(self.x.data_ptr(), self.nlocal, stream=stream)
        else:
            # several ranks: one pack kernel, the all-to-all receives straight into the ghost block of x
            ns = int(dc.send_idx.numel())
            buf = self._msgbuf("_sendbuf", ns)
            self._check(self._md.ani_md_pack_ghosts(self.x.data_ptr(), dc.send_idx.data_ptr(), dc.send_shift.data_ptr(), ns,
                                                    buf.data_ptr(), stream))
            dc._a2a(buf, dc.recv_splits, dc.send_splits, out=self.x[self.nlocal:])

    def _reverse_send(self, stream):
        """first half of the reverse exchange on the device: the ghost rows of f travel to their owners' ranks (one rank: they are
        here already)"""
        dc = self.dc
        if not dc.multi:
            return
        if self.native is not None:
            self.native.reverse_send(self.f.data_ptr(), self.nlocal, stream=stream)
        else:
            dc._a2a(self.f[self.nlocal:], dc.send_splits, dc.recv_splits, out=self._msgbuf("_recvbuf", int(dc.send_idx.numel())))

    def _reverse_unpack(self, stream):
        """second half: what arrived is added into the owners' rows (an atom can be a ghost of several bricks / images)"""
        dc = self.dc
        if not dc.multi:
            self._check(self._md.ani_md_reverse_ghosts(self.f.data_ptr(), dc.send_idx.data_ptr(), self.nlocal,
                                                       self.ntotal - self.nlocal, stream))
        elif self.native is not None:
            self.native.reverse_unpack(self.f.data_ptr(), stream=stream)
        else:
            self._check(self._md.ani_md_unpack_reverse(self.f.data_ptr(), dc.send_idx.data_ptr(), int(dc.send_idx.numel()),
                                                       self._recvbuf.data_ptr(), stream))

    def _reverse_ghosts(self):
        """reverse exchange of the ghost forces on the loop's stream, both halves back to back"""
        if self.dc.multi and self.native is not None:
            self.native.reverse(self.f.data_ptr(), self.nlocal, stream=self._stream)   # both halves; one kernel with one participant
        else:
            self._reverse_send(self._stream)
            self._reverse_unpack(self._stream)

    def _ghosts_and_forces(self, rebuild: bool, sample: bool = False):
        """re-neighbouring or forward ghost positions, then forces and reverse ghost forces, by whichever path the loop is on; then,
        with restraints set, their two launches on the final owned rows of f (sample: this evaluation may write a series row)"""
        if rebuild:
            self._build_list()
            self._forces()
        elif self._overlap:
            self._forces_overlapped()
        else:
            if not self._fold:   # folded: the pack kernel of the step reads the images' positions from their owners (and writes them to x)
                self._forward_ghosts(self._stream)
            self._forces()
        if self._restr is not None:
            self._restraint_forces(sample)

    def minimize(self, etol: float, ftol: float, maxiter: int, dt0=None, check_every=None, on_look=None, **fire_params):
        """``min_style fire`` + ``minimize etol ftol maxiter``: FIRE energy minimisation of the owned atoms without leaving the
        device (ani_md_fire_*, include/ani_md.h).  Velocities are zeroed, then every iteration is the three FIRE launches, ghost
        positions, ani_compute_full_device and ghost forces on the paths of ``run`` (ghost fold, native re-neighbouring,
        device_overwrite_forces).  The optimiser's whole state lives in a device record; the host looks every `check_every`
        iterations (default: the loop's `every`) with the one pinned read of the displacement check, which brings the record
        along: it rebuilds the list when an atom has moved more than skin/2, stops when the record says so, and raises on a
        non-finite energy.  A stopped record freezes x, v and itself, so the result does not depend on `check_every`.
        dt0: first timestep in fs (default: the loop's dt); fire_params: dtmax, dtmin, dtgrow, dtshrink, alpha0, alphashrink,
        delaystep, initialdelay, halfstepback, dmax (defaults of LAMMPS ``min_modify``, ani_hip.fire_params); on_look: optional
        callable(state dict) at every look of the host, before a rebuild.
        Returns a dict: iterations, stop (etol / ftol / maxiter), energy_before / energy_after, fnorm_before / fnorm_after
        (sqrt(sum f.f) over the owned atoms), force_evaluations, uphill_events, limited_moves, rebuilds.
        On return v is zero, the forces belong to the positions, step_no and the Langevin stream are untouched: ``run`` can follow.
        With restraints set (set_restraints) the minimised energy includes the bias and every force evaluation is followed by
        their two launches; no series row is written.
        One rank only: with several, the three sums of an iteration would need an all-reduce each (open lead)."""
        if self.dc.multi:
            raise RuntimeError("VerletRun.minimize: one rank only (the sums of an iteration are not reduced over ranks)")
        if not self._native_rebuild:
            raise RuntimeError("VerletRun.minimize needs the device loop with native re-neighbouring (one rank on the GPU)")
        if self._cons is not None:
            raise RuntimeError("VerletRun.minimize: bond constraints are set (LAMMPS turns SHAKE into restraints during a "
                               "minimisation; that is not built) -- clear them with set_constraints([]) first")
        from . import ani_hip
        md, st, n = self._md, self._stream, self.nlocal
        maxiter = int(maxiter)
        every = self.every if check_every is None else int(check_every)
        if every < 1 or maxiter < 0:
            raise ValueError("VerletRun.minimize: check_every >= 1 and maxiter >= 0")
        par = ani_hip.fire_params(self.dt if dt0 is None else dt0, etol, ftol, maxiter, **fire_params)
        ns = ani_hip.FIRE_NSTATE
        state = torch.zeros(ns, dtype=torch.float64, device=self.device)
        work = torch.empty(md.ani_md_fire_work_size(n), dtype=torch.float64, device=self.device)
        chk_dev = torch.zeros(1 + ns, dtype=torch.float64, device=self.device)
        chk_host = torch.zeros(1 + ns, dtype=torch.float64).pin_memory()
        fm = FTM2V / self.mass[:, 0].contiguous()
        self._check(md.ani_md_fire_init(state.data_ptr(), self.v.data_ptr(), n, par, st))
        builds0 = self.nbuilds
        # the forces of the start point: those in f may carry the thermostat's term of the last step
        self._ghosts_and_forces(False)
        nevals, calls = 1, 0
        while True:
            self._check(md.ani_md_fire_iterate(self.x.data_ptr(), self.v.data_ptr(), self.f.data_ptr(), fm.data_ptr(), n,
                                               self.ev.data_ptr(), par, state.data_ptr(), work.data_ptr(),
                                               self.x_built.data_ptr(), self._d2max.data_ptr(), st))
            calls += 1
            self.since_build += 1
            rebuild = False
            # the stop by maxiter falls in call maxiter + 1 at the latest: that look ends the loop whatever check_every is
            if calls % every == 0 or calls == maxiter + 1:
                worst = self._look(extra=(state, chk_dev, chk_host))
                rec = dict(zip(ani_hip.FIRE_STATE_KEYS, chk_host[1:].tolist()))
                if on_look is not None:
                    on_look(rec)
                if worst == float("inf") or rec["stop"] == 4.0:
                    self.v.zero_()
                    raise RuntimeError("non-finite energy or force norm in VerletRun.minimize: a neighbour count exceeded the "
                                       "kernels' LDS capacity (ANI_ERR_CAPACITY) or the forces diverged")
                if rec["stop"] != 0.0:
                    break
                rebuild = worst > self._d2_rebuild
            self._ghosts_and_forces(rebuild)
            nevals += 1
        self.v.zero_()
        return dict(iterations=int(rec["iterations"]), stop=ani_hip.FIRE_STOP_REASONS[int(rec["stop"])],
                    energy_before=rec["e_first"], energy_after=rec["e_cur"], fnorm_before=rec["ff_first"] ** 0.5,
                    fnorm_after=rec["ff"] ** 0.5, force_evaluations=nevals, uphill_events=int(rec["uphill"]),
                    limited_moves=int(rec["limited"]), rebuilds=self.nbuilds - builds0)

    # ---- Nose-Hoover chain ---------------------------------------------------------------------------------
    def set_nvt(self, t_start, t_stop=None, t_period=None, mtchain: int = 3, nc_tchain: int = 1, drag: float = 0.0):
        """``fix nvt temp t_start t_stop t_period`` (and the `temp` half of ``fix npt``): a Nose-Hoover chain of `mtchain` links at
        constant volume, on the device (ani_md_nh_*, include/ani_md.h), fp64 whatever the handle.  t_stop None: t_start; t_period
        None: 100 dt (fs); nc_tchain: sub-steps of the chain per half-step; drag: as ``fix_modify drag``.  set_nvt(None) clears the
        thermostat: the loop launches what it launched before.  The chain starts at rest.
        Where the chain's half-steps stand in a step: _first_half / _second_half and DESIGN.md §3.5 (the scale factor s stays on the
        device).  3 N - 3 - nb degrees of freedom, nb the constrained bonds as they are when a step runs.
        Every run() and every step() call begins with a fresh ani_md_nh_kinetic of the velocities as they are (LAMMPS
        computes the temperature in setup()), so velocities set by hand, by create_velocities or zeroed by minimize() never leave a
        stale sum in the record; inside a run() the chain goes on from the sum it scaled itself.  step() N times and run(N)
        therefore agree to the rounding of that sum, not bitwise.  In run(N) step k = 1..N has the target t_start + (k / N)
        (t_stop - t_start) in both of its half-steps, every run() ramps anew, afterwards the target stays at t_stop; step() uses the
        current target (t_start before the first run()).  The target is a kernel argument: the host reads nothing.
        Raises with ``langevin``, with several ranks, for a temperature that is not positive and for mtchain outside 1..8."""
        self._clear_npt()             # set_nvt and set_npt clear each other
        if t_start is None:
            self._nvt = None
            return
        from . import ani_hip
        if self.langevin is not None:
            raise RuntimeError("VerletRun.set_nvt: the run has a Langevin thermostat (langevin=...); one temperature control at a time")
        if self.dc.multi:
            raise RuntimeError("VerletRun.set_nvt: one rank only (the kinetic energy is not reduced over ranks)")
        t_start = float(t_start)
        t_stop = t_start if t_stop is None else float(t_stop)
        t_period = 100.0 * self.dt if t_period is None else float(t_period)
        if not (t_start > 0.0 and t_stop > 0.0 and np.isfinite(t_start) and np.isfinite(t_stop)):
            raise ValueError("VerletRun.set_nvt: temperatures must be positive")
        if not 1 <= int(mtchain) <= ani_hip.NH_MAXCHAIN:
            raise ValueError(f"VerletRun.set_nvt: mtchain must be in 1..{ani_hip.NH_MAXCHAIN}")
        if not (t_period > 0.0) or int(nc_tchain) < 1 or drag < 0.0:
            raise ValueError("VerletRun.set_nvt: t_period > 0, nc_tchain >= 1 and drag >= 0")
        if 3 * self.nlocal - 3 - self._ncons <= 0:
            raise ValueError("VerletRun.set_nvt: no degrees of freedom")
        par = ani_hip.NhParams(self.dt, t_period, float(drag), int(mtchain), int(nc_tchain))
        state = torch.zeros(ani_hip.NH_NSTATE, dtype=torch.float64, device=self.device)
        work = torch.empty(self._md.ani_md_nh_work_size(self.nlocal), dtype=torch.float64, device=self.device)
        self._check(self._md.ani_md_nh_init(state.data_ptr(), self._stream))
        self._nvt = dict(t_start=t_start, t_stop=t_stop, t_target=t_start, par=par, state=state, work=work,
                         npart=(self.nlocal + 255) // 256, mass=self.mass[:, 0].contiguous(), mtchain=int(mtchain))

    def _nvt_chain(self, t_target: float, npart: int):
        nvt = self._nvt
        self._check(self._md.ani_md_nh_chain(nvt["state"].data_ptr(), nvt["work"].data_ptr(), npart, t_target,
                                             3.0 * self.nlocal - 3.0 - self._ncons, nvt["par"], self._stream))

    def _nvt_kinetic(self):
        nvt = self._nvt
        self._check(self._md.ani_md_nh_kinetic(self.v.data_ptr(), nvt["mass"].data_ptr(), self.nlocal, nvt["work"].data_ptr(), self._stream))

    def nvt_state(self) -> dict:
        """the chain's device record (one synchronising read): half_steps, k2 (sum m v^2 after the last scaling, kcal/mol), s and
        t_target of the last half-step, ecouple, tdof, nonfinite (half-steps that found a non-finite sum and did nothing), and
        eta, eta_dot, eta_dotdot of the mtchain links"""
        if self._nvt is None:
            raise RuntimeError("VerletRun.nvt_state: no thermostat is set (set_nvt)")
        from .ani_hip import nh_state_dict
        return nh_state_dict(self._nvt["state"].cpu().numpy(), self._nvt["mtchain"])

    # ---- isotropic barostat ----------------------------------------------------------------------------------
    def set_npt(self, t_start, t_stop=None, t_period=None, p_start: float = 1.0, p_stop=None, p_period=None, mtchain: int = 3,
                mpchain: int = 3, nc_tchain: int = 1, nc_pchain: int = 1, drag: float = 0.0):
        """``fix npt temp t_start t_stop t_period iso p_start p_stop p_period``: the isotropic Martyna-Tobias-Klein barostat with a
        chain of `mpchain` links on top of the Nose-Hoover thermostat chain of set_nvt, on the device (ani_md_npt_*,
        include/ani_md.h; `mtk yes`), fp64 whatever the handle.  Pressures in atm; p_stop None: p_start; p_period in fs, None:
        1000 dt; the temperature arguments, nc_tchain and drag as set_nvt.  drag is the thermostat's only: the barostat and its chain
        have none (LAMMPS applies ``fix_modify drag`` to both).  set_npt(None) clears barostat and thermostat: the loop launches what
        it launched before, in the box as it is then.  set_npt and set_nvt clear each other.  Both chains start at rest.
        The box lives in the barostat's device record and changes in every step; a step launches what a thermostatted step launches
        (chain, first half, second half, chain, scale) and never synchronises.  The host's copy of the box (box(), the DomainComm
        geometry, the wrap's and the ghost shell's bounds) is refreshed by every look it takes anyway (the displacement check's
        pinned read brings the record along) and before every re-neighbouring; a re-neighbouring wraps, selects the ghost shell,
        bounds the list and sets the ghost shifts in the box of that moment, and between two of them the shifts are scaled with the
        box.  The displacement check is held against npt_rebuild_limit.  The pressure ramps like the temperature: step k = 1..N of
        run(N) has p_start + (k / N) (p_stop - p_start), afterwards the target stays at p_stop; step() uses the current target.
        thermo() takes volume, ecouple (both chains, the strain rate's kinetic term and p_target (V - V0)) and density from the
        record; minimize() leaves the barostat alone.
        Raises without ``vflag`` (the barostat reads the pair virial of every step), with ``langevin``, with several ranks, without
        native re-neighbouring, while constraints are set (the constraint virial is not accumulated and the constraint kernels take
        the box from the host: the open lead), for temperatures or periods that are not positive, and for mtchain
        or mpchain outside 1..8."""
        if t_start is None:
            self._clear_npt()
            self._nvt = None
            return
        from . import ani_hip
        if not self.vflag:
            raise RuntimeError("VerletRun.set_npt needs vflag=True (the barostat reads the pair virial of every force evaluation)")
        if self.langevin is not None:
            raise RuntimeError("VerletRun.set_npt: the run has a Langevin thermostat (langevin=...); one temperature control at a time")
        if self._recenter is not None:
            raise RuntimeError("VerletRun.set_npt: recentring is set (set_recenter): its target is a fraction of a box at rest -- clear "
                               "it with set_recenter(None) first")
        if self.dc.multi:
            raise RuntimeError("VerletRun.set_npt: one rank only (kinetic energy and virial are not reduced over ranks)")
        if not self._native_rebuild:
            raise RuntimeError("VerletRun.set_npt needs the device loop with native re-neighbouring (one rank on the GPU)")
        if self._cons is not None:
            raise RuntimeError("VerletRun.set_npt: bond constraints are set (the constraint virial is not accumulated and the "
                               "constraint kernels take a host box) -- clear them with set_constraints([]) first")
        p_start = float(p_start)
        p_stop = p_start if p_stop is None else float(p_stop)
        p_period = 1000.0 * self.dt if p_period is None else float(p_period)
        if not (np.isfinite(p_start) and np.isfinite(p_stop)):
            raise ValueError("VerletRun.set_npt: pressures must be finite")
        if not (p_period > 0.0 and np.isfinite(p_period)) or int(nc_pchain) < 1:
            raise ValueError("VerletRun.set_npt: p_period must be positive and nc_pchain >= 1")
        if not 1 <= int(mpchain) <= ani_hip.NH_MAXCHAIN:
            raise ValueError(f"VerletRun.set_npt: mpchain must be in 1..{ani_hip.NH_MAXCHAIN}")
        self.set_nvt(t_start, t_stop, t_period, mtchain, nc_tchain, drag)     # the thermostat's record, scratch and refusals
        nh = self._nvt["par"]
        par = ani_hip.NptParams(self.dt, nh.t_period, nh.drag, p_period, nh.mtchain, nh.nc_tchain, int(mpchain), int(nc_pchain))
        ns = ani_hip.NPT_NSTATE
        state = torch.zeros(ns, dtype=torch.float64, device=self.device)
        self._check(self._md.ani_md_npt_init(state.data_ptr(), self._lo3.ctypes.data, self._len3.ctypes.data, self.nlocal, self._stream))
        self._npt = dict(p_start=p_start, p_stop=p_stop, p_target=p_start, par=par, state=state, mpchain=int(mpchain), fresh=True,
                         chk_dev=torch.zeros(1 + ns, dtype=torch.float64, device=self.device),
                         chk_host=torch.zeros(1 + ns, dtype=torch.float64).pin_memory(),
                         lo_built=self._box_lo_np.copy(), len_built=self._box_len_np.copy(), nimg_max=self.dc.nimg_max)

    def _clear_npt(self):
        """the barostat goes: the host's copy of the box catches up first, the loop goes on in that box (re-neighboured in it, with
        the forces evaluated again, when the box has moved since the last build)"""
        npt = self._npt
        if npt is not None:
            if not npt["fresh"]:
                self._npt_read_box()
            self._npt = None
            # the constant limit of a box at rest measures from the box of the build: a box that has moved since is re-neighboured now
            if (self._box_lo_np != npt["lo_built"]).any() or (self._box_len_np != npt["len_built"]).any():
                self._ghosts_and_forces(True)

    def _npt_chain(self, phase: int, t_target: float, p_target: float, npart: int):
        nvt, npt = self._nvt, self._npt
        self._check(self._md.ani_md_npt_chain(phase, nvt["state"].data_ptr(), npt["state"].data_ptr(), nvt["work"].data_ptr(), npart,
                                              self.ev.data_ptr(), t_target, p_target, 3.0 * self.nlocal - 3.0 - self._ncons,
                                              npt["par"], self._stream))

    def _npt_read_box(self):
        """one synchronising read of the barostat record; the host's copy of the box follows it.  Returns the record."""
        rec = self._npt["state"].cpu().numpy()
        self._set_box(rec[NPT_LAYOUT["lo"]], rec[NPT_LAYOUT["len"]])
        self._npt["fresh"] = True
        return rec

    def npt_state(self) -> dict:
        """the barostat's device record (one synchronising read): half_steps, omega_dot (the strain rate, 1/fs), omega (its time
        integral: ln(L / L0)), press and p_target of the last strain-rate update (atm), W, fv, mu, lo, len, ratio (box and the shift
        ratio of the last first half), c, v0, vol, ecouple (the barostat's part of the conserved quantity), ecouple_chain, nonfinite,
        natoms, and eta, eta_dot, eta_dotdot of the mpchain links"""
        if self._npt is None:
            raise RuntimeError("VerletRun.npt_state: no barostat is set (set_npt)")
        from .ani_hip import npt_state_dict
        return npt_state_dict(self._npt_read_box(), self._npt["mpchain"])

    def box(self):
        """(lo [3], len [3]) of the periodic box as it is now; with a barostat one synchronising read of its record"""
        if self._npt is not None:
            self._npt_read_box()
        return self._box_lo_np.copy(), self._box_len_np.copy()

    # ---- bond constraints ----------------------------------------------------------------------------------
    def set_constraints(self, bonds, lengths=None, tol: float = 1e-10, maxiter: int = 20, project: bool = True):
        """``fix shake`` / ``fix rattle`` on bonds: holonomic bond-length constraints in the RATTLE form (ani_md_shake_positions /
        ani_md_rattle_velocities, include/ani_md.h).  bonds: [nb, 2] global tags; lengths: [nb] in A (None: the current
        minimum-image distances); tol: bound on | |r|^2 - d^2 | / d^2 of every bond after the position stage; maxiter: Newton
        iterations per cluster and step.  The host builds the clusters (``constraint_clusters``: stars of a centre and one to
        three partners, ValueError otherwise).  From here on the two stages stand behind the two halves of every step
        (_first_half / _second_half), in step() and run() alike; every look of the host (the displacement check)
        brings the stage's statistics along and raises when a cluster did not converge.  project: run the position stage once on the positions as they are (old and
        new positions the same, no velocity written), then the velocity stage, and -- with lengths given, which moves atoms --
        evaluate the forces again.  An empty bond list clears the constraints: the loop launches what it launched before.
        temperature() and create_velocities count 3 N - 3 - nb degrees of freedom.  One rank with native re-neighbouring only
        (the owned atoms keep their order there, so the cluster table stays valid across rebuilds)."""
        if self.dc.multi:
            raise RuntimeError("VerletRun.set_constraints: one rank only (a cluster's atoms would have to migrate together)")
        if not self._native_rebuild:
            raise RuntimeError("VerletRun.set_constraints needs the device loop with native re-neighbouring (one rank on the GPU)")
        if self._npt is not None:
            raise RuntimeError("VerletRun.set_constraints: a barostat is set (set_npt): the constraint virial is not accumulated and "
                               "the constraint kernels take a host box")
        from . import ani_hip
        bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
        nb = int(bonds.shape[0])
        if nb == 0:
            self._cons, self._ncons = None, 0
            return
        if not (tol > 0.0) or int(maxiter) < 1:
            raise ValueError("VerletRun.set_constraints: tol > 0 and maxiter >= 1")
        n = self.nlocal
        cl, slot = constraint_clusters(bonds, self.tag.cpu().numpy())
        used = slot >= 0
        if lengths is None:
            x = self.x[:n].cpu().numpy()
            dv = x[np.repeat(cl[:, :1], 3, 1)[used]] - x[cl[:, 1:][used]]
            for k in range(3):
                if self.dc.periodic[k]:
                    dv[:, k] -= self._box_len_np[k] * np.round(dv[:, k] / self._box_len_np[k])
            dused = np.sqrt((dv * dv).sum(1))
        else:
            blen = np.asarray(lengths, dtype=np.float64).reshape(-1)
            if blen.shape[0] != nb:
                raise ValueError(f"VerletRun.set_constraints: {nb} bonds but {blen.shape[0]} lengths")
            dused = blen[slot[used]]
        if not (np.isfinite(dused).all() and (dused > 0.0).all()):
            raise ValueError("VerletRun.set_constraints: bond lengths must be positive and finite")
        d = np.zeros((cl.shape[0], 3))
        d[used] = dused
        # the statistics sit behind the word of the displacement check: one pinned read of a look brings both
        ns = ani_hip.SHAKE_NSTATS
        self._chk_dev = torch.zeros(1 + ns, dtype=torch.float64, device=self.device)
        self._chk_host = torch.zeros(1 + ns, dtype=torch.float64).pin_memory()
        self._cons = dict(cl=torch.as_tensor(cl, device=self.device).contiguous(), d=torch.as_tensor(d, device=self.device).contiguous(),
                          nc=int(cl.shape[0]), tol=float(tol), maxiter=int(maxiter), stats=self._chk_dev[1:])
        self._ncons = nb
        if project:
            self._shake_positions(with_velocities=False)
            self.project_velocities()
            self._constraint_health(self._chk_dev[1:].cpu())
            if lengths is not None:
                self._ghosts_and_forces(False)   # the forces of the projected positions

    def _shake_positions(self, with_velocities: bool = True):
        c = self._cons
        self._check(self._md.ani_md_shake_positions(self.x.data_ptr(), self.v.data_ptr() if with_velocities else None, c["cl"].data_ptr(),
                                                    c["d"].data_ptr(), c["nc"], self._dtfm1.data_ptr(), self.dt, c["tol"], c["maxiter"],
                                                    self._len3.ctypes.data, self._pmask, self.x_built.data_ptr(),
                                                    self._d2max.data_ptr(), c["stats"].data_ptr(), self._stream))

    def project_velocities(self):
        """the velocity stage on the current v: the components along the constrained bonds are taken out (``fix rattle``'s
        half; after velocities were set by hand).  Nothing to do without constraints."""
        c = self._cons
        if c is None:
            return
        self._check(self._md.ani_md_rattle_velocities(self.x.data_ptr(), self.v.data_ptr(), c["cl"].data_ptr(), c["d"].data_ptr(), c["nc"],
                                                      self._dtfm1.data_ptr(), self._len3.ctypes.data, self._pmask, self._stream))

    @staticmethod
    def _stats_record(words) -> dict:
        """the ANI_MD_SHAKE_NSTATS words (a float64 tensor on the host that carries their bit patterns) as a dict"""
        rec = {k: int(w) for k, w in zip(SHAKE_STATS_KEYS, words.numpy().view(np.uint64))}
        rec["max_residual"] = float(np.array(rec["max_residual"], dtype=np.uint64).view(np.float64))
        return rec

    def _constraint_health(self, words):
        rec = self._stats_record(words)
        if rec["unconverged"] != 0 or not np.isfinite(rec["max_residual"]):
            raise RuntimeError(f"bond constraints: {rec['unconverged']} cluster solve(s) reached maxiter = {self._cons['maxiter']} "
                               f"unconverged; largest relative residual {rec['max_residual']:.3e} (tol {self._cons['tol']:.1e}) "
                               f"over {rec['calls']} calls")

    def constraint_stats(self) -> dict:
        """the record of the position stage since set_constraints: unconverged (cluster solves that reached maxiter, summed over
        the calls), max_iterations, max_residual (largest final | |r|^2 - d^2 | / d^2) and calls"""
        if self._cons is None:
            raise RuntimeError("VerletRun.constraint_stats: no constraints are set")
        return self._stats_record(self._chk_dev[1:].cpu())

    # ---- umbrella restraints ---------------------------------------------------------------------------------
    def set_restraints(self, restraints, stride: int = 0, capacity: int = 4096):
        """PLUMED ``DISTANCE`` / ``ANGLE`` / ``TORSION`` + ``RESTRAINT`` (+ ``PRINT STRIDE=stride``), LAMMPS ``fix restrain bond`` /
        ``angle``: harmonic restraints on collective variables (ani_md_restraints_eval / ani_md_restraints_apply, include/ani_md.h),
        fp64 whatever the handle.  restraints: a sequence of (kind, tags, kappa, centre) with kind "distance" (2 global tags),
        "angle" (3, the middle one the apex) or "torsion" (4); kappa >= 0 in kcal/mol/A^2 or kcal/mol/rad^2 (PLUMED's KAPPA=100
        kJ/mol/rad^2 is 23.9006), centre in A or rad.  From here on two launches stand behind every force evaluation -- of step(),
        run() (the one-launch step boundary stays), minimize() and the set-up re-evaluations -- after the ghost forces are folded:
        the bias force is added to f, the bias energy to ev[0] and, with ``vflag``, the bias virial to ev[1..10), so
        potential_energy(), thermo() (pe, press, econserve), virial() and the barostat's strain rate see the bias with no change
        of their own (LAMMPS ``fix_modify energy yes virial yes``).  Under set_npt the restraints take the box from the barostat's
        device record.  This call builds the tables and evaluates the forces again: f, ev and the record belong to the current
        positions.  A restraint that is not finite (a collinear torsion, coincident atoms) makes the energy NaN, and the loop's
        next look raises as for any non-finite energy.
        stride > 0: every step with step_no % stride == 0 -- and the evaluation of this call, when that holds -- writes the row
        step, cv, bias energies into a device buffer of `capacity` rows (the host counts and wraps; restraint_series reads).
        minimize() does not sample.  An empty list clears the restraints: the forces are evaluated again without them and the loop
        launches what it launched before.  One rank with native re-neighbouring only (the owned atoms keep their order there, so
        the tables stay valid across rebuilds).  Raises ValueError for an unknown kind, an unknown tag, a repeated tag inside one
        restraint, a wrong tag count, a negative or non-finite kappa, a non-finite centre, stride < 0 and capacity < 1."""
        if self.dc.multi:
            raise RuntimeError("VerletRun.set_restraints: one rank only (a restraint's atoms would have to migrate together)")
        if not self._native_rebuild:
            raise RuntimeError("VerletRun.set_restraints needs the device loop with native re-neighbouring (one rank on the GPU)")
        from . import ani_hip
        restraints = list(restraints)
        if int(stride) < 0 or int(capacity) < 1:
            raise ValueError("VerletRun.set_restraints: stride >= 0 and capacity >= 1")
        if not restraints:
            had, self._restr = self._restr is not None, None
            if had:
                self._ghosts_and_forces(False)     # f and ev without the bias
            return
        local = {int(t): i for i, t in enumerate(self.tag.cpu().numpy().tolist())}
        nr = len(restraints)
        atoms = np.full((nr, 4), -1, dtype=np.int32)
        kind = np.zeros(nr, dtype=np.int32)
        for r, item in enumerate(restraints):
            try:
                name, tags, _, _ = item
                tags = [int(t) for t in tags]
            except (TypeError, ValueError):
                raise ValueError(f"restraint {r}: expected (kind, tags, kappa, centre), got {item!r}") from None
            if name not in ani_hip.RESTRAINT_KINDS:
                raise ValueError(f"restraint {r}: unknown kind {name!r} (one of {sorted(ani_hip.RESTRAINT_KINDS)})")
            kind[r], want = ani_hip.RESTRAINT_KINDS[name]
            if len(tags) != want:
                raise ValueError(f"restraint {r}: a {name} takes {want} tags, got {len(tags)}")
            for t in tags:
                if t not in local:
                    raise ValueError(f"restraint {r} ({name}): unknown tag {t}")
            if len(set(tags)) != len(tags):
                raise ValueError(f"restraint {r} ({name}): repeated tag in {tuple(tags)}")
            atoms[r, :want] = [local[t] for t in tags]
        kappa, centre = self._restraint_windows([it[3] for it in restraints], [it[2] for it in restraints], nr, "set_restraints")
        touched, row_ptr, entries = ani_hip.restraint_gather_table(atoms)
        dev = self.device

        def ints(a):
            return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev)

        def zeros(*shape):
            return torch.zeros(shape, dtype=torch.float64, device=dev)

        self._restr = dict(nr=nr, nt=int(touched.shape[0]), atoms=ints(atoms), kind=ints(kind), kappa=torch.as_tensor(kappa, device=dev),
                           centre=torch.as_tensor(centre, device=dev), touched=ints(touched), row_ptr=ints(row_ptr), entries=ints(entries),
                           cv=zeros(nr), e=zeros(nr), fslot=zeros(nr, 4, 3), w=zeros(nr, 9), rec=zeros(ani_hip.RESTRAINT_NREC),
                           stride=int(stride), capacity=int(capacity), series=zeros(int(capacity), 1 + 2 * nr) if stride else None,
                           nsamples=0)
        self._ghosts_and_forces(False, sample=True)

    @staticmethod
    def _restraint_windows(centres, kappas, nr: int, where: str):
        """(kappa [nr], centre [nr]) as float64 arrays, checked; kappas None: not given"""
        try:
            centre = np.array([float(c) for c in centres], dtype=np.float64)
            kappa = None if kappas is None else np.array([float(k) for k in kappas], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"VerletRun.{where}: kappa and centre must be numbers") from None
        if centre.shape[0] != nr or (kappa is not None and kappa.shape[0] != nr):
            raise ValueError(f"VerletRun.{where}: {nr} restraints, {centre.shape[0]} centres"
                             + ("" if kappa is None else f", {kappa.shape[0]} kappas"))
        if not np.isfinite(centre).all():
            raise ValueError(f"VerletRun.{where}: every centre must be finite")
        if kappa is not None and not (np.isfinite(kappa).all() and (kappa >= 0.0).all()):
            raise ValueError(f"VerletRun.{where}: every kappa must be finite and >= 0")
        return kappa, centre

    def set_restraint_centres(self, centres, kappas=None):
        """move the windows of the restraints that are set (centres [nr]; kappas [nr] or None: as they are) without rebuilding the
        tables, and evaluate the forces again.  Writes no series row: a step's row holds the window that the step ran in."""
        rs = self._restr
        if rs is None:
            raise RuntimeError("VerletRun.set_restraint_centres: no restraints are set (set_restraints)")
        kappa, centre = self._restraint_windows(centres, kappas, rs["nr"], "set_restraint_centres")
        rs["centre"].copy_(torch.as_tensor(centre))
        if kappa is not None:
            rs["kappa"].copy_(torch.as_tensor(kappa))
        self._ghosts_and_forces(False)

    def _restraint_forces(self, sample: bool):
        """the two launches behind a force evaluation; the box of the moment comes from the barostat's record when there is one"""
        rs, md, st, n = self._restr, self._md, self._stream, self.nlocal
        box_dev = self._npt["state"][NPT_LAYOUT["len"]].data_ptr() if self._npt is not None else None
        self._check(md.ani_md_restraints_eval(self.x.data_ptr(), n, rs["atoms"].data_ptr(), rs["kind"].data_ptr(), rs["kappa"].data_ptr(),
                                              rs["centre"].data_ptr(), rs["nr"], self._len3.ctypes.data, box_dev, self._pmask,
                                              rs["cv"].data_ptr(), rs["e"].data_ptr(), rs["fslot"].data_ptr(), rs["w"].data_ptr(), st))
        row = None
        if sample and rs["stride"] and self.step_no % rs["stride"] == 0:
            row = rs["series"][rs["nsamples"] % rs["capacity"]].data_ptr()
            rs["nsamples"] += 1
        self._check(md.ani_md_restraints_apply(self.f.data_ptr(), n, self.ev.data_ptr(), 1 if self.vflag else 0, rs["touched"].data_ptr(),
                                               rs["row_ptr"].data_ptr(), rs["entries"].data_ptr(), rs["nt"], rs["fslot"].data_ptr(),
                                               rs["cv"].data_ptr(), rs["e"].data_ptr(), rs["w"].data_ptr(), rs["centre"].data_ptr(),
                                               rs["kind"].data_ptr(), rs["nr"], rs["rec"].data_ptr(), float(self.step_no), row, st))

    def restraint_state(self) -> dict:
        """the restraints' device record and outputs of the last evaluation (one synchronising read each): evaluations, ebias (the
        bias energy that is in ev[0]), virial [3, 3], nonfinite, max_delta (largest |cv - centre|, torsions folded), skipped (words of the gather
        table that point outside: always 0 with the table this class builds), and cv [nr], energy [nr]"""
        rs = self._restr
        if rs is None:
            raise RuntimeError("VerletRun.restraint_state: no restraints are set (set_restraints)")
        from .ani_hip import restraint_state_dict
        out = restraint_state_dict(rs["rec"].cpu().numpy())
        out.update(cv=rs["cv"].cpu().numpy(), energy=rs["e"].cpu().numpy())
        return out

    def restraint_series(self, reset: bool = False) -> dict:
        """The rows written so far, in time order: step [ns], cv [ns, nr], ebias [ns, nr], and dropped (rows overwritten because
        more than `capacity` were written since the last reset).  One copy of the buffer; synchronises only here.  reset: start
        an empty series afterwards."""
        rs = self._restr
        if rs is None:
            raise RuntimeError("VerletRun.restraint_series: no restraints are set (set_restraints)")
        nr, cap, ns = rs["nr"], rs["capacity"], rs["nsamples"]
        if rs["series"] is None or ns == 0:
            rows = np.zeros((0, 1 + 2 * nr))
        else:
            buf = rs["series"].cpu().numpy()
            rows = buf[:ns] if ns <= cap else np.concatenate([buf[ns % cap:], buf[: ns % cap]])
        if reset:
            rs["nsamples"] = 0
        return dict(step=rows[:, 0].astype(np.int64), cv=rows[:, 1:1 + nr].copy(), ebias=rows[:, 1 + nr:].copy(), dropped=max(0, ns - cap))

    # ---- centre of mass, momentum, recentring (include/ani_md_protocol.h) -----------------------------------------------------
    def _protocol_guard(self, who: str):
        if self.dc.multi:
            raise RuntimeError(f"VerletRun.{who}: one rank only (the sums are not reduced over ranks)")
        if not self._native_rebuild:
            raise RuntimeError(f"VerletRun.{who} needs the device loop with native re-neighbouring (one rank on the GPU)")

    def _need_images(self, who: str):
        if self._img is None and any(self.dc.periodic):
            raise RuntimeError(f"VerletRun.{who}: a dimension is periodic, and the centre of mass is taken in unwrapped coordinates -- "
                               "call set_images() first")

    def _com_buffers(self):
        if self._com is None:
            from . import ani_hip
            n = self.nlocal
            self._com = dict(mass=self.mass[:, 0].contiguous(), ref=np.zeros(3), target=np.zeros(3),
                             work=torch.empty(self._md.ani_md_com_work_size(n), dtype=torch.float64, device=self.device),
                             rec=torch.zeros(ani_hip.COM_NREC, dtype=torch.float64, device=self.device))
        return self._com

    def _com_sample(self):
        """the record of ani_md_com_sample for the owned atoms as they are, the raw moments taken about the box centre"""
        c = self._com_buffers()
        c["ref"][:] = self._box_lo_np + 0.5 * self._box_len_np
        self._check(self._md.ani_md_com_sample(self.x.data_ptr(), None if self._img is None else self._img.data_ptr(), self.v.data_ptr(),
                                               c["mass"].data_ptr(), self.nlocal, c["ref"].ctypes.data, self._len3.ctypes.data,
                                               self._box_dev()[1], self._pmask, c["work"].data_ptr(), c["rec"].data_ptr(), self._stream))

    def _com_apply(self, flags: int, dim_mask: int = 0):
        c = self._com
        self._check(self._md.ani_md_com_apply(self.x.data_ptr(), self.v.data_ptr(), None if self._img is None else self._img.data_ptr(),
                                              self.nlocal, c["rec"].data_ptr(), flags, c["target"].ctypes.data, dim_mask,
                                              self._len3.ctypes.data, self._box_dev()[1], self._pmask, self.x_built.data_ptr(),
                                              self._d2max.data_ptr(), self._stream))

    def com_state(self) -> dict:
        """Sample now and read (one synchronising read): mass (g/mol), xcm [3] (unwrapped with image flags kept, else of the
        positions as the loop holds them), vcm [3] (A/fs), angmom [3] about xcm (g/mol A^2/fs), inertia [6] about xcm (xx yy zz xy
        xz yz, g/mol A^2), omega [3] (1/fs), singular (1: the inertia tensor has no inverse -- one atom, collinear atoms -- and omega
        is zero), nonfinite (atoms with a non-finite position or velocity) and count."""
        self._protocol_guard("com_state")
        from .ani_hip import com_state_dict
        self._com_sample()
        return com_state_dict(self._com["rec"].cpu().numpy())

    def zero_momentum(self, linear: bool = True, angular: bool = False):
        """``velocity all zero linear`` / ``zero angular``, one pass of ``fix momentum``: one sample and one apply
        (ani_md_com_sample / ani_md_com_apply), nothing read by the host.  angular needs the image flags (set_images) when a
        dimension is periodic."""
        self._protocol_guard("zero_momentum")
        if angular:
            self._need_images("zero_momentum(angular=True)")
        flags = (1 if linear else 0) | (2 if angular else 0)
        if flags:
            self._com_sample()
            self._com_apply(flags)

    def set_momentum(self, every: int, linear: bool = True, angular: bool = False):
        """``fix momentum every linear 1 1 1 [angular]``: at the end of every step with step_no % every == 0 the linear and / or
        angular momentum of the owned atoms is taken out of the full-step velocities (one sample, one apply).  Those steps take the
        separate second half, as step() does; the others keep the one-launch step boundary.  0 clears it: the loop launches what it
        launched before.  angular needs the image flags (set_images) when a dimension is periodic."""
        if int(every) < 0:
            raise ValueError("VerletRun.set_momentum: every >= 0")
        if int(every) == 0:
            self._mom = None
            return
        self._protocol_guard("set_momentum")
        if angular:
            self._need_images("set_momentum(angular=True)")
        flags = (1 if linear else 0) | (2 if angular else 0)
        if not flags:
            raise ValueError("VerletRun.set_momentum: linear, angular or both")
        self._com_buffers()
        self._mom = dict(every=int(every), flags=flags)

    def set_recenter(self, fraction):
        """``fix recenter fx fy fz units fraction``: (fx, fy, fz), None for a dimension that is left alone (LAMMPS' NULL).  Behind the
        first half of every step, and behind the position stage of the constraints, one sample and one apply shift every owned atom
        so that the centre of mass (unwrapped) stands at lo + f len; the shift counts in the displacement check.  None or False
        clears it: the loop launches what it launched before.  Needs the image flags (set_images) when a dimension is periodic;
        raises under set_npt (the target would be a fraction of a moving box)."""
        if fraction is None or fraction is False:
            self._recenter = None
            return
        self._protocol_guard("set_recenter")
        if self._npt is not None:
            raise RuntimeError("VerletRun.set_recenter: a barostat is set (set_npt): the target is a fraction of a box at rest")
        try:
            frac = [None if f is None else float(f) for f in fraction]
        except (TypeError, ValueError):
            raise ValueError("VerletRun.set_recenter: expected (fx, fy, fz) with None for a dimension that is left alone") from None
        if len(frac) != 3 or not all(f is None or np.isfinite(f) for f in frac):
            raise ValueError("VerletRun.set_recenter: expected three finite fractions (None for a dimension that is left alone)")
        self._need_images("set_recenter")
        self._com_buffers()
        self._recenter = dict(frac=frac, dim_mask=sum(1 << k for k in range(3) if frac[k] is not None))

    def _recenter_now(self):
        rc, c = self._recenter, self._com
        for k in range(3):
            c["target"][k] = 0.0 if rc["frac"][k] is None else self._box_lo_np[k] + rc["frac"][k] * self._box_len_np[k]
        self._com_sample()
        self._com_apply(4, rc["dim_mask"])

    # ---- image flags, mean-squared displacements, trajectory frames ---------------------------------------------
    def _transport_guard(self, who: str):
        if self.dc.multi:
            raise RuntimeError(f"VerletRun.{who}: one rank only (the image flags would have to migrate with their atoms)")
        if not self._native_rebuild:
            raise RuntimeError(f"VerletRun.{who} needs the device loop with native re-neighbouring (one rank on the GPU)")

    def _tag_rank(self):
        """(order [n]: the local index of the atom with the k-th smallest global tag; rank [n] int32 on the device: its inverse, where
        atom i goes in a table by tag).  One rank with native re-neighbouring: the owned atoms keep their order, made once."""
        if self._tag_order is None:
            order = np.argsort(self.tag.cpu().numpy(), kind="stable")
            rank = np.empty(self.nlocal, dtype=np.int32)
            rank[order] = np.arange(self.nlocal, dtype=np.int32)
            self._tag_order, self._tag_rank_dev = order, torch.as_tensor(rank, device=self.device)
        return self._tag_order, self._tag_rank_dev

    def _box_dev(self):
        """(lo, len) of the box as device addresses of the barostat record's words, (None, None) without a barostat: the kernels
        then take the host's box"""
        if self._npt is None:
            return None, None
        state = self._npt["state"]
        return state[NPT_LAYOUT["lo"]].data_ptr(), state[NPT_LAYOUT["len"]].data_ptr()

    def set_images(self, on: bool = True):
        """LAMMPS' ``image`` flags: from this call on the wrap of every re-neighbouring (ani_md_wrap_positions_images,
        include/ani_md_transport.h, in place of ani_md_wrap_positions -- the only place the loop wraps: step, run, minimize and the
        rebuilds under the barostat) adds the box lengths it removes from an owned atom to an [nlocal, 3] int32 table, which starts
        at zero: images count from this call.  Calling it again while the table exists changes nothing.  set_images(False) drops the
        table: the loop launches what it launched before; raises while an MSD or a dump is set (they need the flags).  One rank
        with native re-neighbouring only (the owned atoms keep their order there)."""
        self._transport_guard("set_images")
        if not on:
            if self._msd is not None or self._dump is not None:
                raise RuntimeError("VerletRun.set_images(False): an MSD or a dump is set, which read the image flags -- clear them "
                                   "first (set_msd({}), set_dump(0))")
            if self._recenter is not None or (self._mom is not None and self._mom["flags"] & 2):
                raise RuntimeError("VerletRun.set_images(False): recentring or an angular fix momentum is set, which take the centre "
                                   "of mass in unwrapped coordinates -- clear them first (set_recenter(None), set_momentum(0))")
            self._img = None
        elif self._img is None:
            self._img = torch.zeros((self.nlocal, 3), dtype=torch.int32, device=self.device)

    def images(self) -> np.ndarray:
        """the image flags [n, 3] int32 in ascending order of the global tag (``dump custom ... ix iy iz``)"""
        if self._img is None:
            raise RuntimeError("VerletRun.images: no image flags are kept (set_images)")
        return self._img.cpu().numpy()[self._tag_rank()[0]]

    def _unwrap_into(self, out):
        self._check(self._md.ani_md_unwrap(self.x.data_ptr(), self._img.data_ptr(), self.nlocal, self._len3.ctypes.data,
                                           self._box_dev()[1], self._pmask, out.data_ptr(), self._stream))

    def unwrapped_positions(self) -> np.ndarray:
        """x + image * len of the owned atoms (LAMMPS' ``xu``), [n, 3] fp64 in ascending order of the global tag, from ani_md_unwrap
        with the box of the moment (under set_npt the barostat's device record)"""
        if self._img is None:
            raise RuntimeError("VerletRun.unwrapped_positions: no image flags are kept (set_images)")
        out = torch.empty((self.nlocal, 3), dtype=torch.float64, device=self.device)
        self._unwrap_into(out)
        return out.cpu().numpy()[self._tag_rank()[0]]

    def set_msd(self, groups, stride: int = 0, capacity: int = 4096):
        """``compute msd`` (com no and com yes at once) for up to 8 groups against one stored origin (ani_md_msd_sample,
        include/ani_md_transport.h), fp64 whatever the handle.  groups: an ordered dict name -> None (all atoms), a species symbol,
        a list of symbols, or an array of global tags.  The host sorts the atoms into the distinct membership patterns (at most 16
        classes), so overlapping groups cost one pass.  Turns the image flags on (set_images) and stores the unwrapped positions
        of this moment as the origin; reset_msd_origin() stores them again.  msd() samples now.  stride > 0: every step with
        step_no % stride == 0 writes a row, after its positions are final, into a device buffer of `capacity` rows (the host counts
        and wraps; msd_series reads).  minimize() does not sample.  An empty dict clears the MSD: the loop launches what it
        launched before (the image flags stay until set_images(False)).  One rank with native re-neighbouring only.  Raises
        ValueError for more than 8 groups or 16 classes, an unknown species or tag, stride < 0 and capacity < 1."""
        self._transport_guard("set_msd")
        from . import ani_hip
        if int(stride) < 0 or int(capacity) < 1:
            raise ValueError("VerletRun.set_msd: stride >= 0 and capacity >= 1")
        groups = dict(groups)
        if not groups:
            self._msd = None
            return
        if len(groups) > ani_hip.MSD_MAXGROUP:
            raise ValueError(f"VerletRun.set_msd: {len(groups)} groups, at most {ani_hip.MSD_MAXGROUP}")
        n = self.nlocal
        symbols = self.ani.species_symbols()
        species = self.species[:n].cpu().numpy()
        tags = self.tag.cpu().numpy()
        member = np.zeros((len(groups), n), dtype=bool)
        for g, (name, spec) in enumerate(groups.items()):
            if spec is None:
                member[g] = True
                continue
            items = [spec] if isinstance(spec, str) else list(np.asarray(spec).reshape(-1).tolist())
            if items and all(isinstance(it, str) for it in items):
                for sym in items:
                    if sym not in symbols:
                        raise ValueError(f"VerletRun.set_msd: group {name!r}: unknown species {sym!r} (the model has {symbols})")
                    member[g] |= species == symbols.index(sym)
            else:
                try:
                    want = np.array([int(t) for t in items], dtype=np.int64)
                except (TypeError, ValueError):
                    raise ValueError(f"VerletRun.set_msd: group {name!r}: expected None, species symbols or global tags") from None
                missing = np.setdiff1d(want, tags)
                if missing.size:
                    raise ValueError(f"VerletRun.set_msd: group {name!r}: unknown tag {int(missing[0])}")
                member[g] = np.isin(tags, want)
        cls, masks, nclass = ani_hip.msd_classes(member)
        if nclass > ani_hip.MSD_MAXCLASS:
            raise ValueError(f"VerletRun.set_msd: the groups overlap in {nclass} distinct ways, at most {ani_hip.MSD_MAXCLASS} classes")
        nclass = max(nclass, 1)
        mass = self.mass[:, 0].contiguous()
        mass_np = mass.cpu().numpy()
        count = np.array([(cls == c).sum() for c in range(nclass)], dtype=np.int32)
        cmass = np.array([mass_np[cls == c].sum() for c in range(nclass)], dtype=np.float64)
        dev, ng = self.device, len(groups)
        self.set_images(True)
        self._msd = dict(names=list(groups), ngroup=ng, nclass=nclass, cls=torch.as_tensor(cls, device=dev), mass=mass,
                         class_count=torch.as_tensor(count, device=dev), class_mass=torch.as_tensor(cmass, device=dev),
                         group_mask=torch.as_tensor(masks, device=dev),
                         group_count=[int(sum(int(count[c]) for c in range(nclass) if (int(masks[g]) >> c) & 1)) for g in range(ng)],
                         x0u=torch.empty((n, 3), dtype=torch.float64, device=dev),
                         work=torch.empty(self._md.ani_md_msd_work_size(n, nclass), dtype=torch.float64, device=dev),
                         out=torch.zeros((ng, ani_hip.MSD_NOUT), dtype=torch.float64, device=dev), stride=int(stride),
                         capacity=int(capacity), nsamples=0,
                         series=torch.zeros((int(capacity), 1 + ng * ani_hip.MSD_NOUT), dtype=torch.float64, device=dev) if stride else None)
        self.reset_msd_origin()

    def reset_msd_origin(self):
        """the unwrapped positions of this moment become the origin of the MSD"""
        if self._msd is None:
            raise RuntimeError("VerletRun.reset_msd_origin: no MSD is set (set_msd)")
        self._unwrap_into(self._msd["x0u"])

    def _msd_sample(self, series_row):
        ms = self._msd
        self._check(self._md.ani_md_msd_sample(self.x.data_ptr(), self._img.data_ptr(), ms["x0u"].data_ptr(), ms["mass"].data_ptr(),
                                               ms["cls"].data_ptr(), self.nlocal, ms["nclass"], ms["class_count"].data_ptr(),
                                               ms["class_mass"].data_ptr(), ms["group_mask"].data_ptr(), ms["ngroup"],
                                               self._len3.ctypes.data, self._box_dev()[1], self._pmask, ms["work"].data_ptr(),
                                               ms["out"].data_ptr(), float(self.step_no), series_row, self._stream))

    def msd(self) -> dict:
        """sample now (no series row) and read: per group name a dict of msd [4] (x, y, z, total: com no), msd_com [4] (com yes),
        dcm [3] (the displacement of the group's centre of mass), count and nonfinite (atoms whose displacement is not finite; their
        NaN is in the sums).  One synchronising read."""
        if self._msd is None:
            raise RuntimeError("VerletRun.msd: no MSD is set (set_msd)")
        from .ani_hip import msd_dict
        self._msd_sample(None)
        out = self._msd["out"].cpu().numpy()
        return {name: msd_dict(out[g], self._msd["group_count"][g]) for g, name in enumerate(self._msd["names"])}

    def msd_series(self, reset: bool = False) -> dict:
        """The rows written so far, in time order: step [ns], groups: per group name a dict of msd [ns, 4], msd_com [ns, 4],
        dcm [ns, 3] and nonfinite [ns]; rows [ns, ngroup, 12], the raw outputs; and dropped (rows overwritten because more than
        `capacity` were written since the last reset).  One copy of the buffer; synchronises only here.  reset: start an empty
        series afterwards."""
        ms = self._msd
        if ms is None:
            raise RuntimeError("VerletRun.msd_series: no MSD is set (set_msd)")
        from .ani_hip import MSD_LAYOUT, MSD_NOUT
        ng, cap, ns = ms["ngroup"], ms["capacity"], ms["nsamples"]
        if ms["series"] is None or ns == 0:
            rows = np.zeros((0, 1 + ng * MSD_NOUT))
        else:
            buf = ms["series"].cpu().numpy()
            rows = buf[:ns] if ns <= cap else np.concatenate([buf[ns % cap:], buf[: ns % cap]])
        if reset:
            ms["nsamples"] = 0
        per = rows[:, 1:].reshape(-1, ng, MSD_NOUT).copy()
        groups = {name: dict(msd=per[:, g, MSD_LAYOUT["msd"]], msd_com=per[:, g, MSD_LAYOUT["com"]], dcm=per[:, g, MSD_LAYOUT["dcm"]],
                             nonfinite=per[:, g, MSD_LAYOUT["nonfinite"]]) for g, name in enumerate(ms["names"])}
        return dict(step=rows[:, 0].astype(np.int64), groups=groups, rows=per, dropped=max(0, ns - cap))

    def set_dump(self, every: int, path=None, unwrap: bool = False, capacity: int = 64):
        """``dump dcd`` / ``dump custom``: every `every`-th step (step_no % every == 0), after its positions are final, one launch
        (ani_md_frame_pack, include/ani_md_transport.h) packs the owned atoms in ascending order of their global tag as fp32,
        with the box of the moment, into a device ring of `capacity` frames.  A full ring is drained with one device-to-host copy
        and one synchronisation; frames() and close_dump() drain what is there.  path: the drained frames are appended to that
        DCD file (dcd.DCDWriter); None: they are kept on the host for frames().  unwrap: write x + image * len instead of the
        wrapped positions.  Turns the image flags on (set_images).  set_dump(0) closes the file and clears the dump: the loop
        launches what it launched before.  minimize() writes no frame.  One rank with native re-neighbouring only.  Raises
        ValueError for every < 0 and capacity < 1."""
        self._transport_guard("set_dump")
        if int(every) < 0 or int(capacity) < 1:
            raise ValueError("VerletRun.set_dump: every >= 0 and capacity >= 1")
        self.close_dump()
        if int(every) == 0:
            return
        from .dcd import DCDWriter
        n, every, capacity = self.nlocal, int(every), int(capacity)
        self.set_images(True)
        # a frame of the ring: the cell (six doubles), then the [3][n] fp32 block, padded to whole doubles -- one buffer, one copy
        stride = 48 + (12 * n + 7) // 8 * 8
        first = (self.step_no // every + 1) * every
        self._dump = dict(every=every, unwrap=bool(unwrap), capacity=capacity, stride=stride, nring=0, steps=[], kept=[],
                          ring=torch.zeros((capacity, stride), dtype=torch.uint8, device=self.device), row=self._tag_rank()[1],
                          writer=None if path is None else DCDWriter(path, n, first, every, self.dt))

    def _dump_frame(self):
        dp, n = self._dump, self.nlocal
        at = dp["ring"].data_ptr() + dp["nring"] * dp["stride"]
        lo_dev, len_dev = self._box_dev()
        self._check(self._md.ani_md_frame_pack(self.x.data_ptr(), self._img.data_ptr(), n, dp["row"].data_ptr(), self._lo3.ctypes.data,
                                               self._len3.ctypes.data, lo_dev, len_dev, self._pmask, 1 if dp["unwrap"] else 0,
                                               at + 48, at, self._stream))
        dp["steps"].append(self.step_no)
        dp["nring"] += 1
        if dp["nring"] == dp["capacity"]:
            self._drain_dump()

    def _drain_dump(self):
        """the frames of the ring to the host (one copy, which synchronises), then to the file or the kept list"""
        dp, n = self._dump, self.nlocal
        nf = dp["nring"]
        if nf == 0:
            return
        buf = dp["ring"][:nf].cpu().numpy()
        cell = np.ascontiguousarray(buf[:, :48]).view(np.float64)
        xyz = np.ascontiguousarray(buf[:, 48:48 + 12 * n]).view(np.float32).reshape(nf, 3, n)
        for k, step in enumerate(dp["steps"]):
            if dp["writer"] is not None:
                dp["writer"].append(cell[k], xyz[k])
            else:
                dp["kept"].append((step, cell[k].copy(), xyz[k].T.copy()))
        dp["nring"], dp["steps"] = 0, []

    def frames(self, reset: bool = True) -> dict:
        """Drain the ring and return the frames kept on the host (a dump without a path; with a path they are in the file and this
        returns none): step [nf], cell [nf, 6] (lo, then len, of the box at each frame) and xyz [nf, n, 3] fp32 in ascending order
        of the global tag.  reset: forget them afterwards."""
        dp = self._dump
        if dp is None:
            raise RuntimeError("VerletRun.frames: no dump is set (set_dump)")
        self._drain_dump()
        kept = dp["kept"]
        out = dict(step=np.array([k[0] for k in kept], dtype=np.int64),
                   cell=np.array([k[1] for k in kept], dtype=np.float64).reshape(-1, 6),
                   xyz=np.array([k[2] for k in kept], dtype=np.float32).reshape(-1, self.nlocal, 3))
        if reset:
            dp["kept"] = []
        return out

    def close_dump(self):
        """drain the ring, close the DCD file and clear the dump; returns what frames() would have returned (None when no dump was
        set)"""
        if self._dump is None:
            return None
        out = self.frames()
        if self._dump["writer"] is not None:
            self._dump["writer"].close()
        self._dump = None
        return out

    def _forces_overlapped(self):
        """Forward exchange, PairANI::compute and reverse exchange of a step that keeps its list, the two exchanges on the
        communication stream: the forward one beside the rows without ghosts (pack, compaction, AEV forward), the reverse
        one beside their backward pass (ani_step_begin / ani_step_ghosts_ready / ani_step_finish)."""
        s1, s2, ev = torch.cuda.current_stream(self.device), self._comm_stream, self._ev
        nl, nt = self.nlocal, self.ntotal
        ev[0].record(s1)                                   # initial_integrate has moved the owned atoms
        with torch.cuda.stream(s2):
            s2.wait_event(ev[0])
            self._forward_ghosts(torch.cuda.current_stream(self.device).cuda_stream)
            ev[1].record(s2)
        self.ani.step_begin(nt, nl, self.x.data_ptr(), self.f.data_ptr(), self.ev.data_ptr(), stream=s1.cuda_stream)
        s1.wait_event(ev[1])                               # ghost positions are in place
        self.ani.step_ghosts_ready(stream=s1.cuda_stream)
        ev[2].record(s1)                                   # ghost rows of f are final
        with torch.cuda.stream(s2):
            s2.wait_event(ev[2])
            self._reverse_send(s2.cuda_stream)
            ev[3].record(s2)
        self.ani.step_finish(stream=s1.cuda_stream)
        s1.wait_event(ev[3])
        self._reverse_unpack(s1.cuda_stream)   # one rank: the owners are here, the ghost rows are added once the owned rows are written

    def _final_integrate(self):
        # fix langevin post_force + fix nve final_integrate
        lang = self._g1 is not None
        self._check(self._md.ani_md_final_integrate(self.v.data_ptr(), self.f.data_ptr(), self._dtfm1.data_ptr(), self.nlocal,
                                                    1 if lang else 0, self._g1.data_ptr() if lang else None,
                                                    self._g2.data_ptr() if lang else None, self.tag.data_ptr(), self._seed,
                                                    self.step_no, self._stream))

    def warm_paths(self):
        """Run once, without touching the trajectory, the pieces of the loop that only some steps execute — the displacement
        check with its host round trip — so that their first-use costs (module loads of the tensor kernels, lazily made
        buffers) fall before a caller's timed region whatever its number of warm-up steps."""
        # not on the loop's own maximum: a look zeroes its word
        self._look(word=torch.zeros(1, dtype=torch.float64, device=self.device))

    # ---- analysis ----------------------------------------------------------------------------------------
    def find_molecules(self, formula_cap: int = 4096):
        """Which molecules are in the box now (ani_find_molecules_device, include/ani_hip.h; the handle needs a bond table:
        ``ani.set_bond_table``): the loop's own positions, the installed list and the owner maps of its ghost shell, on the loop's
        stream.  Returns (mol_of_atom [nlocal] int32, {formula string: count}, summary int64 [6]) like ANI.find_molecules.  One
        rank only: merging the open molecules of several ranks is not done here (the summary's open counts are what such an
        exchange would start from)."""
        if self.dc.multi:
            raise RuntimeError("VerletRun.find_molecules: one rank only (molecules that cross ranks are not merged)")
        from .ani_hip import AniError, formula_dict
        n, ng, st = self.nlocal, self.ntotal - self.nlocal, self._stream
        owner = self.dc.send_idx
        if ng:
            self._forward_ghosts(st)   # the ghost rows of x as images of the owned atoms' positions of this moment
        S = len(self.ani.species_symbols())
        mol = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        rows = torch.zeros((int(formula_cap), S + 1), dtype=torch.int32, device=self.device)
        summ = torch.zeros(6, dtype=torch.int64, device=self.device)
        self.ani.find_molecules_device(self.ntotal, n, self.x.data_ptr(), owner.data_ptr() if ng else None, mol.data_ptr(),
                                       rows.data_ptr(), int(formula_cap), summ.data_ptr(), stream=st)
        summ = summ.cpu().numpy()
        if summ[1] > formula_cap:
            raise AniError(f"find_molecules: {int(summ[1])} distinct compositions, formula_cap is {formula_cap}")
        return mol[:n].cpu().numpy(), formula_dict(rows[: int(summ[1])].cpu().numpy(), self.ani.species_symbols()), summ

    def set_rdf(self, pairs, nbins: int = 100, rmax=None, every: int = 1):
        """``compute rdf`` + ``fix ave/time``: radial distribution functions accumulated on the device (ani_rdf_*,
        include/ani_hip.h).  pairs: ordered (centre, neighbour) species pairs as symbols or indices, [("O", "O"), ("O", "H"), ...];
        nbins bins on [0, rmax), rmax None = the loop's force cutoff (cutneigh - skin; never above the model's radial cutoff).
        From here on every step with step_no % every == 0 adds one frame right after its force evaluation: one launch on the
        loop's stream with the loop's own positions, no host synchronisation.  minimize() does not sample.  An empty `pairs`
        clears the RDF: the loop launches what it launched before.  Calling it again discards what was accumulated.  One rank
        only: the per-rank counts are summable, the sum over ranks is not built."""
        if self.dc.multi:
            raise RuntimeError("VerletRun.set_rdf: one rank only (the ranks' counts are not summed)")
        if pairs is None or len(pairs) == 0:
            self._rdf_every = 0
            self.ani.rdf_configure(1, 1.0, None)
            return
        if int(every) < 1:
            raise ValueError("VerletRun.set_rdf: every >= 1")
        # a refused configuration raises here and changes nothing: what was set before goes on
        self.ani.rdf_configure(int(nbins), self.cutneigh - self.skin if rmax is None else float(rmax), pairs)
        self._rdf_every = int(every)

    def sample_rdf(self):
        """one frame now, on the current positions (whatever `every` says)"""
        if self.ani.rdf_config() is None:
            raise RuntimeError("VerletRun.sample_rdf: no RDF is set (set_rdf)")
        if self.ntotal > self.nlocal:
            self._forward_ghosts(self._stream)   # the ghost rows of x as images of the owned atoms' positions of this moment
        self.ani.rdf_accumulate_device(self.ntotal, self.nlocal, self.x.data_ptr(), stream=self._stream)

    def rdf(self, reset: bool = False) -> dict:
        """Read and normalise what was accumulated (ani_hip.rdf_normalise: r, g, coord), plus the raw counts [npair, nbins],
        centres [npair], frames, and pairs [npair, 2].  Species counts from the owned atoms, the volume from the box.  reset:
        zero the accumulators afterwards.  With a barostat the volume is that of the box at the time of this read: LAMMPS'
        ``compute rdf`` normalises every frame with the volume of its own moment, which is not built."""
        from .ani_hip import rdf_normalise
        cfg = self.ani.rdf_config()
        if cfg is None:
            raise RuntimeError("VerletRun.rdf: no RDF is set (set_rdf)")
        nbins, rmax, pairs = cfg
        counts, centres, frames = self.ani.rdf_read(reset=reset)
        n_of = np.bincount(self.species[: self.nlocal].cpu().numpy(), minlength=len(self.ani.species_symbols()))
        out = rdf_normalise(counts, centres, nbins, rmax, pairs, n_of, float(np.prod(self.box()[1])))
        out.update(counts=counts, centres=centres, frames=frames, pairs=pairs.copy())
        return out

    # ---- thermo ------------------------------------------------------------------------------------------
    def kinetic_energy(self) -> float:
        ke = 0.5 * MVV2E * (self.mass * self.v.square()).sum().reshape(1)
        return self._allreduce_sum(ke.clone())

    def potential_energy(self) -> float:
        """ev[0] of the last force evaluation summed over ranks: the model's energy plus, with restraints set, their bias"""
        return self._allreduce_sum(self.ev[:1].clone())

    def virial(self) -> np.ndarray:
        """the pair style's virial of the last force evaluation, summed over ranks (kcal/mol, row-major 3x3; needs vflag)"""
        if not self.vflag:
            raise RuntimeError("VerletRun was made without vflag")
        return self._allreduce(self.ev[1:10].clone(), "sum").cpu().numpy().reshape(3, 3)

    def thermo(self) -> dict:
        """``thermo_style custom pe ke etotal temp press vol density`` from the device: one ani_md_thermo call (include/ani_md.h)
        and one read.  Keys: pe, ke, etotal (kcal/mol), temp (K, on 3 N - 3 - nb degrees of freedom), press and pxx pyy pzz pxy pxz
        pyz (atm: kinetic tensor plus the pair virial of the last force evaluation, over the box volume), vol (A^3), density
        (g/cm^3), ecouple (the chain's energy, 0 without set_nvt; with set_npt the barostat's part as well, and vol and density follow the
        box of the record) and econserve = etotal + ecouple.  The pressure entries are NaN
        without ``vflag``, and while constraints are set (the constraint virial is not accumulated).  With restraints set
        (set_restraints) pe, etotal and econserve include the bias energy and the pressure entries the bias virial.  One rank on
        the device.  The first call also sums the masses for the density, once."""
        if self.dc.multi:
            raise RuntimeError("VerletRun.thermo: one rank only (the sums are not reduced over ranks)")
        from . import ani_hip
        n = self.nlocal
        if self._thermo_buf is None or self._thermo_buf["n"] != n:
            mass = self.mass[:, 0].contiguous()
            self._thermo_buf = dict(n=n, mass=mass, mtot=float(mass.sum()),
                                    work=torch.empty(self._md.ani_md_thermo_work_size(n), dtype=torch.float64, device=self.device),
                                    out=torch.zeros(ani_hip.THERMO_N, dtype=torch.float64, device=self.device))
        b = self._thermo_buf
        npt_rec = self._npt_read_box() if self._npt is not None else None
        vol = float(np.prod(self._box_len_np)) if npt_rec is None else float(npt_rec[NPT_LAYOUT["vol"]])
        self._check(self._md.ani_md_thermo(self.v.data_ptr(), b["mass"].data_ptr(), n, self.ev.data_ptr(),
                                           1 if (self.vflag and self._cons is None) else 0, 3.0 * n - 3.0 - self._ncons, vol,
                                           self._nvt["state"].data_ptr() if self._nvt is not None else None, b["work"].data_ptr(),
                                           b["out"].data_ptr(), self._stream))
        rec = dict(zip(ani_hip.THERMO_KEYS, b["out"].cpu().tolist()))
        del rec["k2"]
        if npt_rec is not None:       # the barostat's part: chain, strain rate and p_target (V - V0)
            rec["ecouple"] += float(npt_rec[NPT_LAYOUT["ecouple"]])
            rec["econserve"] = rec["etotal"] + rec["ecouple"]
        rec["density"] = b["mtot"] / vol / 0.602214129      # g/mol/A^3 -> g/cm^3 (LAMMPS units real, mv2d)
        return rec

    def temperature(self, natoms_all: int) -> float:
        """LAMMPS compute temp: 2 KE / ((3 N - 3 - nb) k_B), nb the constrained bonds (set_constraints; 0 without)"""
        return 2.0 * self.kinetic_energy() / ((3.0 * natoms_all - 3.0 - self._ncons) * BOLTZ)
