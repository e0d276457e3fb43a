"""ctypes binding of the C ABI in include/ani_hip.h (libani_hip.so).

Mirrors the reference's ``class ANI`` (src/ani_csrc/ani.h:11-85): construct with the pair_style arguments, call
``compute`` each step with ``ago`` telling whether the neighbour list was rebuilt.  There is no CPU fallback:
if the library is missing or no GPU is visible this raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
# ANI_HIP_LIB selects an alternative build of the same library (kernel A/B experiments); never a different backend
LIB_PATH = os.environ.get("ANI_HIP_LIB") or os.path.join(_CSRC, "libani_hip.so")
HARTREE2KCALMOL = 627.5094738898777

EXPORTS = ["ani_create", "ani_destroy", "ani_last_error", "ani_num_models", "ani_use_num_models", "ani_num_species",
           "ani_aev_length", "ani_cutoff_radial", "ani_cutoff_angular", "ani_compute_full", "ani_compute_half",
           "ani_compute_full_device", "ani_build_list_device", "ani_build_list", "ani_debug_list", "ani_debug_get", "ani_debug_read", "ani_debug_colmap", "ani_debug_stream_tables", "ani_set_option", "ani_phase_timing", "ani_phase_times",
           "ani_trace_push", "ani_trace_pop", "ani_trace_mark", "ani_step_begin", "ani_step_ghosts_ready", "ani_step_finish",
           "ani_debug_fused_stamps", "ani_attach_comm", "ani_debug_fused_schedule", "ani_debug_fused_schedule_halves", "ani_last_mlp_kernel", "ani_last_repulsion_kernel", "ani_host_register", "ani_host_unregister", "ani_set_ghost_fold", "ani_stage_ghost_fold",
           "ani_request_atom_virial", "ani_request_model_deviation", "ani_debug_deviation_parts",
           "ani_set_bond_table", "ani_find_molecules_device", "ani_find_molecules", "ani_species_symbol",
           "ani_rdf_configure", "ani_rdf_accumulate_device", "ani_rdf_accumulate", "ani_rdf_read"]
# include/ani_comm.h: the device-side ghost exchange over RCCL
COMM_EXPORTS = ["ani_comm_get_unique_id", "ani_comm_create", "ani_comm_create_local", "ani_comm_destroy", "ani_comm_last_error", "ani_comm_rank",
                "ani_comm_size", "ani_comm_plan", "ani_comm_exchange_counts", "ani_comm_alltoallv", "ani_comm_set_epoch",
                "ani_comm_set_epoch_host", "ani_comm_set_ghost_order", "ani_comm_forward", "ani_comm_reverse", "ani_comm_reverse_send", "ani_comm_reverse_unpack",
                "ani_comm_allreduce_f64", "ani_comm_set_option", "ani_comm_get_stat"]


class AniError(RuntimeError):
    pass


class DebugView(C.Structure):
    _fields_ = [("nlocal", C.c_int), ("ntotal", C.c_int), ("nrows", C.c_int), ("npairs", C.c_int64),
                ("d_aev", C.c_void_p), ("d_gaev", C.c_void_p), ("d_row_of_centre", C.c_void_p),
                ("species_count", C.c_int * 16), ("aev_stride", C.c_int), ("aev_active_length", C.c_int), ("error_flags", C.c_int)]


class StreamTablesView(C.Structure):
    """ani_stream_tables_view of include/ani_hip.h"""
    _fields_ = [("species", C.c_int32), ("bound", C.c_int32), ("tuples", C.c_int32), ("builds", C.c_int32),
                ("words_bwd", C.c_int64), ("words_fwd", C.c_int64), ("d_words_bwd", C.c_void_p), ("d_words_fwd", C.c_void_p),
                ("build_ms", C.c_double)]


class FireParams(C.Structure):
    """ani_md_fire_params of include/ani_md.h"""
    _fields_ = [(n, C.c_double) for n in ("dt0", "dtmax", "dtmin", "dtgrow", "dtshrink", "alpha0", "alphashrink", "dmax", "etol",
                                          "ftol")] + [(n, C.c_int) for n in ("delaystep", "initialdelay", "halfstepback", "maxiter")]


# The device records of include/ani_md.h, one table per record: field -> its index, or the slice of a field of several words.  A field
# is the header's enum member without its prefix (ANI_MD_NPT_OMEGA_DOT is NPT_LAYOUT["omega_dot"]; "P" and "W" are written as the
# dicts below have always spelt them); tests/test_abi_exports.py holds the tables against the header.  "zero" words are padding.
FIRE_NSTATE = 16
FIRE_LAYOUT = dict(iterations=0, dt=1, alpha=2, last_negative=3, e_prev=4, e_cur=5, P=6, vv=7, ff=8, dtv=9, uphill=10, limited=11,
                   stop=12, e_first=13, ff_first=14, vmax=15)
FIRE_STATE_KEYS = tuple(FIRE_LAYOUT)
FIRE_STOP_REASONS = ("running", "etol", "ftol", "maxiter", "non-finite")
# ANI_MD_SHAKE_NSTATS words of include/ani_md.h (ani_md_shake_positions): the third is the bit pattern of a double
SHAKE_NSTATS = 4
SHAKE_STATS_KEYS = ("unconverged", "max_iterations", "max_residual", "calls")
# the Nose-Hoover chain's state record and the thermo record of include/ani_md.h (ani_md_nh_*, ani_md_thermo)
NH_NSTATE = 32
NH_MAXCHAIN = 8
NH_LAYOUT = dict(half_steps=0, k2=1, s=2, t_target=3, ecouple=4, tdof=5, nonfinite=6, zero=7, eta=slice(8, 16), eta_dot=slice(16, 24),
                 eta_dotdot=slice(24, 32))
THERMO_N = 16
THERMO_LAYOUT = dict(pe=0, ke=1, temp=2, press=3, pxx=4, pyy=5, pzz=6, pxy=7, pxz=8, pyz=9, etotal=10, ecouple=11, econserve=12, vol=13,
                     k2=14, zero=15)
THERMO_KEYS = tuple(k for k in THERMO_LAYOUT if k != "zero")


class NhParams(C.Structure):
    """ani_md_nh_params of include/ani_md.h"""
    _fields_ = [("dt", C.c_double), ("t_period", C.c_double), ("drag", C.c_double), ("mtchain", C.c_int), ("nc_tchain", C.c_int)]


def _record_dict(rec, layout, nlinks: int) -> dict:
    """a record (host array) by its layout table: one-word fields as floats, longer ones as copies, of a chain's eta, eta_dot and
    eta_dotdot the first nlinks links; padding left out"""
    rec = np.asarray(rec, dtype=np.float64)
    out = {}
    for name, at in layout.items():
        if name == "zero":
            continue
        if name.startswith("eta"):
            at = slice(at.start, at.start + nlinks)
        out[name] = rec[at].copy() if isinstance(at, slice) else float(rec[at])
    return out


def nh_state_dict(rec, mtchain: int = NH_MAXCHAIN) -> dict:
    """the ANI_MD_NH_NSTATE doubles of a chain record (host array) as a dict; eta, eta_dot, eta_dotdot: the first mtchain links"""
    return _record_dict(rec, NH_LAYOUT, mtchain)


# the barostat record of include/ani_md.h (ani_md_npt_*)
NPT_NSTATE = 56
NPT_LAYOUT = dict(half_steps=0, omega_dot=1, omega=2, press=3, p_target=4, W=5, fv=6, mu=7, lo=slice(8, 11), len=slice(11, 14),
                  ratio=slice(14, 17), c=slice(17, 20), v0=20, ecouple=21, nonfinite=22, natoms=23, eta=slice(24, 32),
                  eta_dot=slice(32, 40), eta_dotdot=slice(40, 48), ecouple_chain=48, vol=49)


class NptParams(C.Structure):
    """ani_md_npt_params of include/ani_md.h"""
    _fields_ = [("dt", C.c_double), ("t_period", C.c_double), ("drag", C.c_double), ("p_period", C.c_double), ("mtchain", C.c_int),
                ("nc_tchain", C.c_int), ("mpchain", C.c_int), ("nc_pchain", C.c_int)]


def npt_state_dict(rec, mpchain: int = NH_MAXCHAIN) -> dict:
    """the ANI_MD_NPT_NSTATE doubles of a barostat record (host array) as a dict; eta, eta_dot, eta_dotdot: the first mpchain links
    of the barostat chain"""
    return _record_dict(rec, NPT_LAYOUT, mpchain)


# the restraint record and the kinds of include/ani_md.h (ani_md_restraints_*): kind -> (code, atoms)
RESTRAINT_NREC = 16
RESTRAINT_LAYOUT = dict(evaluations=0, ebias=1, virial=slice(2, 11), nonfinite=11, max_delta=12, skipped=13, zero=slice(14, 16))
RESTRAINT_KINDS = {"distance": (0, 2), "angle": (1, 3), "torsion": (2, 4)}


def restraint_gather_table(atoms):
    """The gather table of ani_md_restraints_apply from atoms [nr, 4] (local indices, -1 unused): (touched [nt] ascending,
    row_ptr [nt + 1], entries: the words 4 restraint + slot of each touched atom, ascending), all int32."""
    atoms = np.asarray(atoms, dtype=np.int64).reshape(-1, 4)
    words = np.flatnonzero(atoms.reshape(-1) >= 0)                 # 4 restraint + slot, ascending
    owner = atoms.reshape(-1)[words]
    order = np.argsort(owner, kind="stable")
    touched, counts = np.unique(owner, return_counts=True)
    row_ptr = np.concatenate([[0], np.cumsum(counts)])
    return touched.astype(np.int32), row_ptr.astype(np.int32), words[order].astype(np.int32)


def restraint_state_dict(rec) -> dict:
    """the ANI_MD_RESTRAINT_NREC doubles of a restraint record (host array) as a dict"""
    out = _record_dict(rec, RESTRAINT_LAYOUT, 0)
    out["virial"] = out["virial"].reshape(3, 3)
    for name in ("evaluations", "nonfinite", "skipped"):
        out[name] = int(out[name])
    return out


# include/ani_md_transport.h: the outputs of ani_md_msd_sample per group (the header's ANI_MD_MSD_* enum), and its limits
MSD_MAXCLASS = 16
MSD_MAXGROUP = 8
MSD_NOUT = 12
MSD_LAYOUT = dict(msd=slice(0, 4), com=slice(4, 8), dcm=slice(8, 11), nonfinite=11)


def msd_classes(membership):
    """The classes of ani_md_msd_sample from membership [ngroup, n] (bool: atom i belongs to group g): the distinct membership
    patterns, numbered in the order of their first atom.  Returns (cls [n] int32, -1 for an atom in no group; group_mask [ngroup]
    int32, bit c set when class c belongs to the group; nclass)."""
    member = np.asarray(membership, dtype=bool)
    ngroup, n = member.shape
    pattern = (member.astype(np.int64) << np.arange(ngroup, dtype=np.int64)[:, None]).sum(0)
    cls = np.full(n, -1, dtype=np.int32)
    masks = np.zeros(ngroup, dtype=np.int64)
    seen = {}
    for i in np.flatnonzero(pattern).tolist():
        c = seen.setdefault(int(pattern[i]), len(seen))
        cls[i] = c
    for pat, c in seen.items():
        for g in range(ngroup):
            if (pat >> g) & 1:
                masks[g] |= 1 << c
    return cls, masks.astype(np.int32), len(seen)


def msd_dict(row, count: int) -> dict:
    """the ANI_MD_MSD_NOUT doubles of one group (host array) as a dict: msd [4], msd_com [4], dcm [3], count, nonfinite"""
    row = np.asarray(row, dtype=np.float64)
    return dict(msd=row[MSD_LAYOUT["msd"]].copy(), msd_com=row[MSD_LAYOUT["com"]].copy(), dcm=row[MSD_LAYOUT["dcm"]].copy(),
                count=int(count), nonfinite=int(row[MSD_LAYOUT["nonfinite"]]))


# include/ani_md_protocol.h: the centre-of-mass record (ANI_MD_COM_*) and the flags of ani_md_com_apply;
# tests/test_protocol_reference_cpu.py holds the table against the header
COM_NREC = 24
COM_LAYOUT = dict(mass=0, xcm=slice(1, 4), vcm=slice(4, 7), angmom=slice(7, 10), inertia=slice(10, 16), omega=slice(16, 19), singular=19,
                  nonfinite=20, count=21, zero=slice(22, 24))
COM_FLAG_LINEAR, COM_FLAG_ANGULAR, COM_FLAG_RECENTER = 1, 2, 4


def com_state_dict(rec) -> dict:
    """the ANI_MD_COM_NREC doubles of a centre-of-mass record (host array) as a dict; inertia: xx yy zz xy xz yz"""
    out = _record_dict(rec, COM_LAYOUT, 0)
    for name in ("singular", "nonfinite", "count"):
        out[name] = int(out[name])
    return out


def fire_params(dt0, etol, ftol, maxiter, **kw) -> FireParams:
    """ani_md_fire_params with the defaults of LAMMPS `min_modify` (dtmax = 10 dt0, dtmin = 0.02 dt0, ...); kw overrides them"""
    vals = dict(dt0=float(dt0), dtmax=10.0 * dt0, dtmin=0.02 * dt0, dtgrow=1.1, dtshrink=0.5, alpha0=0.25, alphashrink=0.99,
                dmax=0.1, etol=float(etol), ftol=float(ftol), delaystep=20, initialdelay=1, halfstepback=1, maxiter=int(maxiter))
    unknown = set(kw) - set(vals)
    if unknown:
        raise TypeError(f"unknown FIRE parameter(s): {sorted(unknown)}")
    vals.update(kw)
    p = FireParams()
    for name, ctype in FireParams._fields_:
        setattr(p, name, int(vals[name]) if ctype is C.c_int else float(vals[name]))
    return p


def build(force: bool = False) -> str:
    """Compile libani_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU).  force: rebuild every object
    (make -B) whatever the timestamps say.  Returns the library path; build.last_commands holds the compiler command
    lines make ran (empty when everything was up to date)."""
    args = ["make", "-C", _CSRC, "-j8"]
    if force:
        args.append("-B")
    out = subprocess.run(args, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    build.last_commands = [ln for ln in out.splitlines() if ln.lstrip().startswith(("hipcc", "g++", "gcc"))]
    return LIB_PATH


build.last_commands = []


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AniError(f"{LIB_PATH} is missing: build it (python -c 'import __graft_entry__ as g; g.build()'); "
                           "there is no fallback path")
        L = C.CDLL(LIB_PATH)
        L.ani_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.ani_destroy.argtypes = [C.c_void_p]
        L.ani_last_error.restype = C.c_char_p
        L.ani_last_error.argtypes = [C.c_void_p]
        for n in ("ani_num_models", "ani_use_num_models", "ani_num_species", "ani_aev_length"):
            getattr(L, n).argtypes = [C.c_void_p]
        for n in ("ani_cutoff_radial", "ani_cutoff_angular"):
            getattr(L, n).argtypes = [C.c_void_p]
            getattr(L, n).restype = C.c_double
        L.ani_compute_full.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
        L.ani_compute_half.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
        L.ani_compute_full_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ani_step_begin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
        L.ani_step_ghosts_ready.argtypes = [C.c_void_p, C.c_void_p]
        L.ani_step_finish.argtypes = [C.c_void_p, C.c_void_p]
        L.ani_build_list_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double,
                                            C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
        L.ani_build_list.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                     C.c_void_p, C.POINTER(C.c_int64)]
        L.ani_debug_list.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3
        L.ani_debug_get.argtypes = [C.c_void_p, C.POINTER(DebugView)]
        L.ani_debug_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.ani_debug_colmap.argtypes = [C.c_void_p, C.c_void_p]
        L.ani_debug_stream_tables.argtypes = [C.c_void_p, C.POINTER(StreamTablesView)] + [C.c_void_p] * 4
        L.ani_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.ani_last_mlp_kernel.argtypes = [C.c_void_p]
        L.ani_set_ghost_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ani_stage_ghost_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.ani_request_atom_virial.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.ani_request_model_deviation.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        L.ani_debug_deviation_parts.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.ani_set_bond_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.ani_find_molecules_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_void_p]
        L.ani_find_molecules.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p]
        L.ani_species_symbol.argtypes = [C.c_void_p, C.c_int]
        L.ani_species_symbol.restype = C.c_char_p
        L.ani_rdf_configure.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int]
        L.ani_rdf_accumulate_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.ani_rdf_accumulate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ani_rdf_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.ani_host_register.argtypes = [C.c_void_p, C.c_size_t]
        L.ani_host_unregister.argtypes = [C.c_void_p]
        L.ani_last_mlp_kernel.restype = C.c_char_p
        L.ani_last_repulsion_kernel.argtypes = [C.c_void_p]
        L.ani_last_repulsion_kernel.restype = C.c_char_p
        # include/ani_md.h: kernels of the LAMMPS-free timestep loop (not part of the drop-in boundary)
        L.ani_md_initial_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
        L.ani_md_final_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.ani_md_final_initial_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]
        L.ani_md_wrap_positions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ani_md_ghost_shell_count.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        L.ani_md_ghost_shell_fill.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
        L.ani_md_append_ghosts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ani_md_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ani_md_forward_ghosts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ani_md_reverse_ghosts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ani_md_reverse_ghosts_ordered.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ani_md_pack_ghosts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ani_md_unpack_reverse.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ani_md_fire_work_size.argtypes = [C.c_int]
        L.ani_md_fire_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(FireParams), C.c_void_p]
        L.ani_md_fire_iterate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(FireParams),
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ani_md_fire_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ani_md_shake_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double,
                                             C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ani_md_rattle_velocities.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_void_p]
        L.ani_md_nh_work_size.argtypes = [C.c_int]
        L.ani_md_nh_init.argtypes = [C.c_void_p, C.c_void_p]
        L.ani_md_nh_kinetic.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ani_md_nh_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.POINTER(NhParams), C.c_void_p]
        L.ani_md_nh_scale.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ani_md_nh_initial_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
        L.ani_md_nh_final_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ani_md_thermo_work_size.argtypes = [C.c_int]
        L.ani_md_thermo.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        L.ani_md_npt_init.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ani_md_npt_chain.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double,
                                       C.c_double, C.POINTER(NptParams), C.c_void_p]
        L.ani_md_npt_initial_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ani_md_npt_final_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
        L.ani_md_npt_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ani_md_restraints_eval.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ani_md_restraints_apply.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        # include/ani_md_transport.h: image flags, unwrapped positions, mean-squared displacements, trajectory frames
        L.ani_md_wrap_positions_images.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ani_md_unwrap.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ani_md_msd_work_size.argtypes = [C.c_int, C.c_int]
        L.ani_md_msd_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_double, C.c_void_p, C.c_void_p]
        L.ani_md_frame_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        # include/ani_md_protocol.h: centre of mass, momentum, recentring
        L.ani_md_com_work_size.argtypes = [C.c_int]
        L.ani_md_com_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ani_md_com_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        # include/ani_comm.h
        L.ani_comm_get_unique_id.argtypes = [C.c_void_p]
        L.ani_comm_create.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.ani_comm_destroy.argtypes = [C.c_void_p]
        L.ani_comm_last_error.restype = C.c_char_p
        L.ani_comm_last_error.argtypes = [C.c_void_p]
        L.ani_comm_rank.argtypes = [C.c_void_p]
        L.ani_comm_size.argtypes = [C.c_void_p]
        L.ani_comm_plan.argtypes = [C.c_int] + [C.c_void_p] * 6
        L.ani_comm_exchange_counts.argtypes = [C.c_void_p] * 4
        L.ani_comm_alltoallv.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
        L.ani_comm_set_epoch.argtypes = [C.c_void_p] * 5
        L.ani_comm_set_ghost_order.argtypes = [C.c_void_p, C.c_void_p]
        L.ani_comm_set_epoch_host.argtypes = [C.c_void_p] * 6
        L.ani_attach_comm.argtypes = [C.c_void_p, C.c_void_p]
        L.ani_md_gather_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ani_md_scatter_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ani_comm_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ani_comm_reverse.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ani_comm_reverse_send.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ani_comm_reverse_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ani_comm_allreduce_f64.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ani_comm_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.ani_comm_get_stat.argtypes = [C.c_void_p, C.c_char_p]
        L.ani_comm_get_stat.restype = C.c_longlong
        L.ani_phase_timing.argtypes = [C.c_void_p, C.c_int]
        L.ani_phase_times.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        _lib = L
    return _lib


def formula_string(counts, symbols) -> str:
    """Formula of a composition in Hill order -- C, then H, then the other symbols alphabetically -- a count of 1 not printed,
    species with a count of 0 left out: formula_string([4, 1, 0, 0], ["H", "C", "N", "O"]) == "CH4"."""
    pairs = [(str(sym), int(n)) for sym, n in zip(symbols, counts) if int(n) > 0]
    pairs.sort(key=lambda p: (0, "") if p[0] == "C" else (1, "") if p[0] == "H" else (2, p[0]))
    return "".join(sym if n == 1 else f"{sym}{n}" for sym, n in pairs)


SUMMARY_KEYS = ("molecules", "compositions", "open_molecules", "bonds", "largest", "open_atoms")


def formula_dict(rows, symbols) -> dict:
    """{formula string: count} of formula rows [n][S + 1] (compositions that print alike are added up)"""
    out = {}
    for row in rows:
        k = formula_string(row[:-1], symbols)
        out[k] = out.get(k, 0) + int(row[-1])
    return out


def rdf_normalise(counts, centres, nbins, rmax, pairs, n_of_species, volume) -> dict:
    """The accumulators of ani_rdf_read as radial distribution functions, normalised like LAMMPS ``compute rdf``.  Pure numpy.
    counts [npair, nbins] and centres [npair] (any frames summed), pairs [npair, 2] species indices (a, b), n_of_species[s] the
    number of atoms of species s in the box, volume in A^3.  Returns a dict:
      r      [nbins]         bin centres
      g      [npair, nbins]  counts[p, k] / (centres[p] * rho_b * 4 pi / 3 * (r_hi^3 - r_lo^3)), rho_b = (N_b - delta_ab) / volume
      coord  [npair, nbins]  cumsum(counts[p]) / centres[p]: the running coordination number
    A pair with centres[p] == 0 or rho_b == 0 gives zeros, not NaN."""
    nbins = int(nbins)
    counts = np.asarray(counts, dtype=np.float64).reshape(-1, nbins)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n_of = np.asarray(n_of_species, dtype=np.float64)
    assert counts.shape[0] == centres.shape[0] == pairs.shape[0]
    edges = np.arange(nbins + 1, dtype=np.float64) * (float(rmax) / nbins)
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    g, coord = np.zeros_like(counts), np.zeros_like(counts)
    for p, (a, b) in enumerate(pairs.tolist()):
        if centres[p] == 0:
            continue
        coord[p] = np.cumsum(counts[p]) / centres[p]
        rho_b = (n_of[b] - (1.0 if a == b else 0.0)) / float(volume)
        if rho_b > 0:
            g[p] = counts[p] / (centres[p] * rho_b * shell)
    return dict(r=0.5 * (edges[1:] + edges[:-1]), g=g, coord=coord)


class ANI:
    """``ANI(model_file, local_rank, use_num_models, use_cuaev, use_fullnbr, use_single)`` — src/ani_csrc/ani.h:31-36."""

    def __init__(self, model_file: str, local_rank: int = 0, use_num_models: int = -1, use_cuaev: bool = True,
                 use_fullnbr: bool = True, use_single: bool = True):
        self._lib = lib()
        self._h = C.c_void_p()
        rc = self._lib.ani_create(model_file.encode(), local_rank, use_num_models, int(use_cuaev), int(use_fullnbr),
                                  int(use_single), C.byref(self._h))
        if rc != 0:
            raise AniError(f"ani_create failed ({rc}): {self._lib.ani_last_error(None).decode()}")
        self.use_cuaev, self.use_fullnbr, self.use_single = use_cuaev, use_fullnbr, use_single
        self.num_models = self._lib.ani_num_models(self._h)
        self.use_num_models = self._lib.ani_use_num_models(self._h)
        self.aev_length = self._lib.ani_aev_length(self._h)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ani_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise AniError(f"libani_hip error {rc}: {self._lib.ani_last_error(self._h).decode()}")

    def request_atom_virial(self, out, ncomp: int):
        """ani_request_atom_virial: arm the NEXT step's per-atom virial into ``out`` (host array or device address, [ntotal, ncomp]
        float64; ncomp 9 = cvatom order, 6 = vatom); None disarms."""
        if isinstance(out, np.ndarray):
            assert out.dtype == np.float64 and out.flags.c_contiguous and out.size == out.shape[0] * ncomp
            out = out.ctypes.data
        self._check(self._lib.ani_request_atom_virial(self._h, out, int(ncomp)))

    DEVIATION_KEYS = ("member_energy", "atom_energy_dev", "member_dforce", "atom_force_dev", "summary")

    def request_model_deviation(self, member_energy=None, atom_energy_dev=None, member_dforce=None, atom_force_dev=None,
                                summary=None):
        """ani_request_model_deviation: arm the NEXT step's ensemble deviation (include/ani_hip.h).  Each output is a C-contiguous
        float64 numpy array (host entry points) or a device address (device entry point); None leaves it out, all None disarms."""
        ptrs = []
        for a in (member_energy, atom_energy_dev, member_dforce, atom_force_dev, summary):
            if isinstance(a, np.ndarray):
                assert a.dtype == np.float64 and a.flags.c_contiguous
                a = a.ctypes.data
            ptrs.append(a)
        self._check(self._lib.ani_request_model_deviation(self._h, *ptrs))

    def debug_deviation_parts(self):
        """(device address, member stride in elements) of the last force-armed step's dg_m rows (ani_debug_deviation_parts)."""
        p, n = C.c_void_p(), C.c_int64()
        self._check(self._lib.ani_debug_deviation_parts(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def compute(self, inp, ago: int = 0, eflag_atom: bool = True, vflag: bool = True, force_into=None, atom_virial: int = 0,
                deviation: bool = False):
        """Host-pointer entry points with a harness.RankInput (full or half list).  Returns a dict like the oracle's.
        force_into: a C-contiguous float64 [ntotal, 3] array handed over as out_force (option out_force_accumulate adds into it).
        atom_virial: 6 or 9 adds "atom_virial" [ntotal, atom_virial] (kcal/mol, include/ani_hip.h), 0 = not asked for.
        deviation: adds "deviation", a dict of the ensemble deviation (include/ani_hip.h): member_energy [M], atom_energy_dev
        [nlocal] and member_dforce [ntotal, M, 3] always, atom_force_dev [nlocal] and summary [4] when the input has no ghosts."""
        nt, nl = inp.ntotal, inp.nlocal
        av = None
        if atom_virial:
            av = np.full((nt, int(atom_virial)), np.nan)
            self.request_atom_virial(av, int(atom_virial))
        dv = None
        if deviation:
            M = self.use_num_models
            dv = dict(member_energy=np.full(M, np.nan), atom_energy_dev=np.full(nl, np.nan), member_dforce=np.full((nt, M, 3), np.nan))
            if nt == nl:
                dv.update(atom_force_dev=np.full(nl, np.nan), summary=np.full(4, np.nan))
            self.request_model_deviation(**dv)
        species = np.ascontiguousarray(inp.species, dtype=np.int64)
        x = np.ascontiguousarray(inp.x, dtype=np.float64)
        e = np.zeros(1)
        f = np.full((nt, 3), np.nan) if force_into is None else force_into
        assert f.dtype == np.float64 and f.shape == (nt, 3) and f.flags.c_contiguous
        ea = np.zeros(nl)
        vir = np.zeros(9)
        if inp.half:
            a12 = np.ascontiguousarray(inp.atom_index12(), dtype=np.int64)
            rc = self._lib.ani_compute_half(self._h, nt, nl, species.ctypes.data, x.ctypes.data, inp.npairs,
                                            a12.ctypes.data, ago, int(eflag_atom), int(vflag), e.ctypes.data,
                                            f.ctypes.data, ea.ctypes.data, vir.ctypes.data)
        else:
            il = np.ascontiguousarray(inp.ilist, dtype=np.int32)
            nn = np.ascontiguousarray(inp.numneigh, dtype=np.int32)
            jl = np.ascontiguousarray(inp.jlist, dtype=np.int32)
            rc = self._lib.ani_compute_full(self._h, nt, nl, species.ctypes.data, x.ctypes.data, inp.npairs,
                                            il.ctypes.data, jl.ctypes.data, nn.ctypes.data, ago, int(eflag_atom),
                                            int(vflag), e.ctypes.data, f.ctypes.data, ea.ctypes.data, vir.ctypes.data)
        self._check(rc)
        out = dict(energy=float(e[0]), force=f, eatom=ea, virial=vir.reshape(3, 3))
        if av is not None:
            out["atom_virial"] = av
        if dv is not None:
            out["deviation"] = dv
        return out

    def compute_device(self, ntotal, nlocal, d_species, d_x, npairs, d_ilist, d_jlist, d_numneigh, ago, d_f, d_ev,
                       d_eatom=None, eflag_atom=False, vflag=False, stream=None, d_atom_virial=None, ncomp=9, d_deviation=None):
        """Device-resident step; arguments are raw device addresses (e.g. torch tensor .data_ptr()).  d_atom_virial: device
        [ntotal, ncomp] float64 the per-atom virial is ADDED to (include/ani_hip.h), None = not asked for.  d_deviation: a dict
        of device addresses keyed like request_model_deviation's arguments, the ensemble deviation is written there."""
        if d_atom_virial is not None:
            self.request_atom_virial(d_atom_virial, ncomp)
        if d_deviation is not None:
            self.request_model_deviation(**d_deviation)
        rc = self._lib.ani_compute_full_device(self._h, ntotal, nlocal, d_species, d_x, npairs, d_ilist, d_jlist,
                                               d_numneigh, ago, int(eflag_atom), int(vflag), d_f, d_ev, d_eatom, stream)
        self._check(rc)

    def step_begin(self, ntotal, nlocal, d_x, d_f, d_ev, d_eatom=None, eflag_atom=False, vflag=False, stream=None,
                   d_atom_virial=None, ncomp=9):
        """Split device-resident step, part 1 of 3 (include/ani_hip.h): needs the owned atoms' positions only.
        d_atom_virial: as for compute_device; step_finish writes it."""
        if d_atom_virial is not None:
            self.request_atom_virial(d_atom_virial, ncomp)
        self._check(self._lib.ani_step_begin(self._h, ntotal, nlocal, d_x, int(eflag_atom), int(vflag), d_f, d_ev, d_eatom, stream))

    def step_ghosts_ready(self, stream=None):
        """Part 2: the ghost positions are in place; afterwards the ghost rows of the force array are final."""
        self._check(self._lib.ani_step_ghosts_ready(self._h, stream))

    def step_finish(self, stream=None):
        """Part 3: forces of the owned atoms, energy, virial."""
        self._check(self._lib.ani_step_finish(self._h, stream))

    def build_list_device(self, ntotal, nlocal, d_species, d_x, cutneigh, lo, hi, stream=None) -> int:
        """Device-side full neighbour list (ani_build_list_device); returns the pair count.  Follow with
        ``compute_device(..., ago=1)`` and null list pointers."""
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        n = C.c_int64()
        self._check(self._lib.ani_build_list_device(self._h, ntotal, nlocal, d_species, d_x, float(cutneigh),
                                                    lo.ctypes.data, hi.ctypes.data, C.byref(n), stream))
        return n.value

    def build_list(self, species, x, nlocal: int, cutneigh: float, lo=None, hi=None) -> int:
        """Host-array form (ani_build_list): species[ntotal], x[ntotal,3] with owned atoms first; returns the pair
        count.  Follow with the host-pointer compute at ago != 0."""
        species = np.ascontiguousarray(species, dtype=np.int64)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if lo is None:   # per column: numpy's axis-0 reduction of an [n,3] array is ~10x slower
            lo = [x[:, k].min() - 0.25 for k in range(3)]
        if hi is None:
            hi = [x[:, k].max() + 0.25 for k in range(3)]
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        n = C.c_int64()
        self._check(self._lib.ani_build_list(self._h, x.shape[0], nlocal, species.ctypes.data, x.ctypes.data, float(cutneigh),
                                             lo.ctypes.data, hi.ctypes.data, C.byref(n)))
        return n.value

    def debug_list(self, nlocal: int):
        """(numneigh[nlocal], jlist[npairs]) of the list installed in the handle, as host arrays."""
        pn, po, pj = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._lib.ani_debug_list(self._h, C.byref(pn), C.byref(po), C.byref(pj)))
        nn = self.debug_read(pn, (nlocal,), np.int32)
        if nlocal == 0:
            return nn, np.zeros(0, np.int32)
        # dense segments, or rows of a fixed capacity (the one-kernel build): gathered into dense segments here
        off = self.debug_read(po, (nlocal + 1,), np.int32)
        span = self.debug_read(pj, (int((off[:-1] + nn).max()),), np.int32)
        if np.array_equal(off[1:] - off[:-1], nn):
            return nn, span[: int(nn.sum())]
        idx = np.repeat(off[:-1] - np.concatenate([[0], np.cumsum(nn)[:-1]]), nn) + np.arange(int(nn.sum()))
        return nn, span[idx]

    def debug_view(self) -> DebugView:
        v = DebugView()
        self._check(self._lib.ani_debug_get(self._h, C.byref(v)))
        return v

    def debug_read(self, d_ptr, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        self._check(self._lib.ani_debug_read(self._h, d_ptr, out.ctypes.data, out.nbytes))
        return out

    def stream_tables(self, contents: bool = True) -> dict:
        """ani_debug_stream_tables: the view's fields and, with `contents`, desc_bwd / desc_fwd [tuples][4] (first word, stream
        length, buckets, words reserved) and words_bwd / words_fwd (uint32) as host arrays; species == 0: the epoch has no tables."""
        v = StreamTablesView()
        self._check(self._lib.ani_debug_stream_tables(self._h, C.byref(v), None, None, None, None))
        out = {n: getattr(v, n) for n, _ in StreamTablesView._fields_}
        if contents and v.species:
            db, df = np.zeros((v.tuples, 4), np.int32), np.zeros((v.tuples, 4), np.int32)
            wb, wf = np.zeros(max(v.words_bwd, 1), np.uint32), np.zeros(max(v.words_fwd, 1), np.uint32)
            self._check(self._lib.ani_debug_stream_tables(self._h, C.byref(v), db.ctypes.data, wb.ctypes.data, df.ctypes.data,
                                                          wf.ctypes.data))
            out.update(desc_bwd=db, words_bwd=wb[: v.words_bwd], desc_fwd=df, words_fwd=wf[: v.words_fwd])
        return out

    def colmap(self) -> np.ndarray:
        v = self.debug_view()
        out = np.zeros(v.aev_active_length, dtype=np.int32)
        self._check(self._lib.ani_debug_colmap(self._h, out.ctypes.data))
        return out

    def set_option(self, name: str, value: int):
        self._check(self._lib.ani_set_option(self._h, name.encode(), int(value)))

    def set_ghost_fold(self, d_owner, d_shift, nghost: int, stream=None):
        """ani_set_ghost_fold: device addresses of owner[nghost] (int64) and shift[nghost][3] (float64); None clears"""
        self._check(self._lib.ani_set_ghost_fold(self._h, d_owner, d_shift, int(nghost), stream))

    def stage_ghost_fold(self, d_owner, d_shift, nghost: int):
        """ani_stage_ghost_fold: the fold of the list the NEXT build_list* call builds (checked behind that build's synchronisation)"""
        self._check(self._lib.ani_stage_ghost_fold(self._h, d_owner, d_shift, int(nghost)))

    def species_symbols(self):
        """the model file's species symbols, in species order (ani_species_symbol)"""
        return [self._lib.ani_species_symbol(self._h, s).decode() for s in range(self._lib.ani_num_species(self._h))]

    def set_bond_table(self, table):
        """ani_set_bond_table: an [S][S] array of bond lengths in Angstrom (<= 0: never bonded), or a dict
        {("H", "O"): 1.16, ...} of unordered symbol pairs (pairs left out are never bonded); None clears the table."""
        if table is None:
            self._check(self._lib.ani_set_bond_table(self._h, None, 0))
            return
        if isinstance(table, dict):
            sym = self.species_symbols()
            t = np.zeros((len(sym), len(sym)))
            for (a, b), v in table.items():
                if a not in sym or b not in sym:
                    raise AniError(f"set_bond_table: the model has no species {a if a not in sym else b!r} (it has {sym})")
                t[sym.index(a), sym.index(b)] = t[sym.index(b), sym.index(a)] = float(v)
            table = t
        t = np.ascontiguousarray(table, dtype=np.float64)
        if t.ndim != 2 or t.shape[0] != t.shape[1]:
            raise AniError(f"set_bond_table: a square table is needed, got shape {t.shape}")
        self._check(self._lib.ani_set_bond_table(self._h, t.ctypes.data, int(t.shape[0])))

    def find_molecules(self, inp_or_x, owner=None, formula_cap: int = 4096, nlocal=None):
        """ani_find_molecules on the installed list.  inp_or_x: a harness.RankInput (its positions), or an [ntotal, 3] array with
        ``nlocal`` (default: all of it).  owner: int64 [nghost], the owned atom every ghost stands for (outside [0, nlocal):
        foreign); None uses an installed ghost fold, or counts every ghost as foreign.  Returns (mol_of_atom [nlocal] int32,
        {formula string: count} of the closed molecules, summary int64 [6] in the order of SUMMARY_KEYS).  More than formula_cap distinct
        compositions raise AniError (ANI_ERR_CAPACITY)."""
        if hasattr(inp_or_x, "nlocal"):
            x, nl = inp_or_x.x, inp_or_x.nlocal
        else:
            x = inp_or_x
            nl = len(x) if nlocal is None else int(nlocal)
        x = np.ascontiguousarray(x, dtype=np.float64)
        nt = x.shape[0]
        S = self._lib.ani_num_species(self._h)
        own = None
        if owner is not None:
            own = np.ascontiguousarray(owner, dtype=np.int64)
            assert own.shape == (nt - nl,)
        mol = np.full(nl, -1, dtype=np.int32)
        rows = np.zeros((int(formula_cap), S + 1), dtype=np.int32)
        summ = np.zeros(6, dtype=np.int64)
        self._check(self._lib.ani_find_molecules(self._h, nt, nl, x.ctypes.data, own.ctypes.data if own is not None else None,
                                                 mol.ctypes.data, rows.ctypes.data, int(formula_cap), summ.ctypes.data))
        return mol, formula_dict(rows[: int(summ[1])], self.species_symbols()), summ

    def find_molecules_device(self, ntotal, nlocal, d_x, d_owner=None, d_mol_of_atom=None, d_formula=None, formula_cap: int = 0,
                              d_summary=None, stream=None):
        """ani_find_molecules_device: raw device addresses (e.g. torch tensor .data_ptr()); any output may be None; nothing
        synchronises.  d_x float64 [ntotal, 3], d_owner int64 [nghost], d_mol_of_atom int32 [nlocal], d_formula int32
        [formula_cap, S + 1] (rows in unspecified order), d_summary int64 [6]."""
        self._check(self._lib.ani_find_molecules_device(self._h, int(ntotal), int(nlocal), d_x, d_owner, d_mol_of_atom, d_formula,
                                                        int(formula_cap), d_summary, stream))

    def rdf_configure(self, nbins: int, rmax: float, pairs):
        """ani_rdf_configure: npair histograms of nbins bins on [0, rmax) A.  pairs: ordered (centre, neighbour) species pairs as
        indices or symbols, [("O", "O"), ("O", "H"), ...]; None or an empty list clears the configuration.  Reconfiguring discards
        what was accumulated."""
        if pairs is None or len(pairs) == 0:
            self._check(self._lib.ani_rdf_configure(self._h, int(nbins), float(rmax), None, 0))
            self._rdf = None
            return
        sym = None
        idx = []
        for pr in pairs:
            a, b = pr
            for v in (a, b):
                if isinstance(v, str):
                    sym = sym or self.species_symbols()
                    if v not in sym:
                        raise AniError(f"rdf_configure: the model has no species {v!r} (it has {sym})")
                    v = sym.index(v)
                idx.append(int(v))
        p = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, 2)
        self._check(self._lib.ani_rdf_configure(self._h, int(nbins), float(rmax), p.ctypes.data, int(p.shape[0])))
        self._rdf = (int(nbins), float(rmax), p)

    def rdf_config(self):
        """(nbins, rmax, pairs int32 [npair, 2]) of the last accepted rdf_configure, None when nothing is configured"""
        return getattr(self, "_rdf", None)

    def rdf_accumulate(self, inp_or_x, nlocal=None):
        """ani_rdf_accumulate: one frame on the installed list.  inp_or_x: a harness.RankInput (its positions), or an [ntotal, 3]
        array with ``nlocal`` (default: all of it)."""
        if hasattr(inp_or_x, "nlocal"):
            x, nl = inp_or_x.x, inp_or_x.nlocal
        else:
            x = inp_or_x
            nl = len(x) if nlocal is None else int(nlocal)
        x = np.ascontiguousarray(x, dtype=np.float64)
        self._check(self._lib.ani_rdf_accumulate(self._h, int(x.shape[0]), int(nl), x.ctypes.data))

    def rdf_accumulate_device(self, ntotal, nlocal, d_x, stream=None):
        """ani_rdf_accumulate_device: d_x is the device address of float64 [ntotal, 3]; nothing synchronises"""
        self._check(self._lib.ani_rdf_accumulate_device(self._h, int(ntotal), int(nlocal), d_x, stream))

    def rdf_read(self, reset: bool = False):
        """ani_rdf_read: (counts uint64 [npair, nbins], centres uint64 [npair], frames int); reset zeroes the accumulators after
        the copy and keeps the configuration"""
        cfg = self.rdf_config()
        if cfg is None:
            raise AniError("rdf_read: nothing is configured (rdf_configure)")
        nbins, _, p = cfg
        counts = np.zeros((p.shape[0], nbins), dtype=np.uint64)
        centres = np.zeros(p.shape[0], dtype=np.uint64)
        frames = np.zeros(1, dtype=np.uint64)
        self._check(self._lib.ani_rdf_read(self._h, counts.ctypes.data, centres.ctypes.data, frames.ctypes.data, int(bool(reset))))
        return counts, centres, int(frames[0])

    def last_mlp_kernel(self) -> str:
        return self._lib.ani_last_mlp_kernel(self._h).decode()

    def last_repulsion_kernel(self) -> str:
        """ani_last_repulsion_kernel: "aev_backward_fast", "repulsion_kernel<float>", "repulsion_kernel<double>", or "" (no block / no step yet)"""
        return self._lib.ani_last_repulsion_kernel(self._h).decode()

    def cutoffs(self):
        """(Rcr, Rca) of the model"""
        return float(self._lib.ani_cutoff_radial(self._h)), float(self._lib.ani_cutoff_angular(self._h))

    def attach_comm(self, comm):
        """ani_attach_comm: a NativeComm (or None) whose reverse exchange the host-pointer entry points run on the device"""
        self._comm_keep = comm
        self._check(self._lib.ani_attach_comm(self._h, comm._h if comm is not None else None))

    def phase_timing(self, enable):
        """1/True: fresh accumulation; 0/False: stop recording; 2: resume without clearing."""
        self._check(self._lib.ani_phase_timing(self._h, int(enable)))

    def phase_times(self):
        ms = (C.c_double * 5)()
        n = C.c_int()
        self._check(self._lib.ani_phase_times(self._h, ms, C.byref(n)))
        return dict(aev_fwd=ms[0], mlp=ms[1], aev_bwd=ms[2], other=ms[3], compact=ms[4], calls=n.value)


def comm_plan(send_counts, recv_counts):
    """ani_comm_plan: (send_off, recv_off, nsend, nrecv) of an all-to-all with these per-peer counts.  Host arithmetic
    only: works without a GPU."""
    sc = np.ascontiguousarray(send_counts, dtype=np.int64)
    rc = np.ascontiguousarray(recv_counts, dtype=np.int64)
    so, ro = np.zeros_like(sc), np.zeros_like(rc)
    ns, nr = C.c_int64(), C.c_int64()
    if lib().ani_comm_plan(len(sc), sc.ctypes.data, rc.ctypes.data, so.ctypes.data, ro.ctypes.data, C.addressof(ns), C.addressof(nr)) != 0:
        raise AniError("ani_comm_plan: bad counts")
    return so, ro, ns.value, nr.value


class NativeComm:
    """include/ani_comm.h: the ghost exchange between ranks as grouped ncclSend / ncclRecv inside libani_hip.so (no torch on
    the data path).  ``id_bytes``: the 128 bytes rank 0 got from ``NativeComm.unique_id()``, handed to every rank by the
    caller (``from_torch`` does it with torch.distributed, the python loop's bootstrap)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_char * 128)()
        if lib().ani_comm_get_unique_id(buf) != 0:
            raise AniError("ani_comm_get_unique_id: " + lib().ani_comm_last_error(None).decode())
        return bytes(buf)

    @classmethod
    def from_torch(cls, device_index: int, group=None):
        """bootstrap over an initialised torch.distributed group (any backend): rank 0's id is broadcast as an object.
        Every rank runs the SAME sequence of collectives whatever fails where: rank 0 broadcasts (status, id) even when it
        could not make an id, and the ranks agree on the outcome of ani_comm_create before anybody uses the communicator --
        so a caller's fallback to another transport is taken by all ranks or by none."""
        import torch.distributed as dist
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        rank = dist.get_rank(group) if dist.is_initialized() else 0
        box = [None]
        if rank == 0:
            try:
                box = [("ok", cls.unique_id())]
            except Exception as e:   # librccl missing, ncclGetUniqueId failed: the peers must hear about it
                box = [("error", str(e))]
        if world > 1:
            dist.broadcast_object_list(box, src=0, group=group)
        status, payload = box[0]
        if status != "ok":
            raise AniError(f"rank 0 could not make an RCCL id: {payload}")
        comm, err = None, None
        try:
            comm = cls(world, rank, payload, device_index)
        except AniError as e:
            err = e
        if world > 1:
            oks = [None] * world
            dist.all_gather_object(oks, err is None, group=group)
            if not all(oks):
                if comm is not None:
                    comm.close()
                raise AniError(f"ani_comm_create failed on rank(s) {[r for r, ok in enumerate(oks) if not ok]}"
                               + (f": {err}" if err is not None else ""))
        elif err is not None:
            raise err
        return comm

    def __init__(self, nranks: int, rank: int, id_bytes: bytes, device_index: int = 0):
        self._lib = lib()
        self._h = C.c_void_p()
        buf = C.create_string_buffer(id_bytes, 128)
        rc = self._lib.ani_comm_create(nranks, rank, buf, device_index, C.byref(self._h))
        if rc != 0:
            raise AniError(f"ani_comm_create failed ({rc}): {self._lib.ani_comm_last_error(None).decode()}")
        self.world, self.rank = nranks, rank
        self._keep = ()

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ani_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise AniError(f"ani_comm error {rc}: {self._lib.ani_comm_last_error(self._h).decode()}")

    def set_option(self, name: str, value: int):
        self._check(self._lib.ani_comm_set_option(self._h, name.encode(), int(value)))

    def stat(self, name: str) -> int:
        """ani_comm_get_stat: 'forward_exchanges', 'reverse_exchanges', 'alltoalls', 'broken' """
        return int(self._lib.ani_comm_get_stat(self._h, name.encode()))

    def exchange_counts(self, send_counts, stream=None):
        sc = np.ascontiguousarray(send_counts, dtype=np.int64)
        rc = np.zeros_like(sc)
        self._check(self._lib.ani_comm_exchange_counts(self._h, sc.ctypes.data, rc.ctypes.data, stream))
        return rc.tolist()

    def alltoallv(self, d_send, send_counts, d_recv, recv_counts, item_bytes: int, stream=None):
        sc = np.ascontiguousarray(send_counts, dtype=np.int64)
        rc = np.ascontiguousarray(recv_counts, dtype=np.int64)
        self._check(self._lib.ani_comm_alltoallv(self._h, d_send, sc.ctypes.data, d_recv, rc.ctypes.data, int(item_bytes), stream))

    def set_epoch(self, send_counts, recv_counts, send_idx, send_shift):
        """send_idx (int64) / send_shift (float64 [n,3]): device tensors; kept alive here until the next epoch"""
        sc = np.ascontiguousarray(send_counts, dtype=np.int64)
        rc = np.ascontiguousarray(recv_counts, dtype=np.int64)
        self._keep = (send_idx, send_shift)
        self._check(self._lib.ani_comm_set_epoch(self._h, sc.ctypes.data, rc.ctypes.data, send_idx.data_ptr(), send_shift.data_ptr()))

    def set_ghost_order(self, ghost_of):
        """ghost_of (int64 device tensor, or None): entry k of the rank-grouped message order is ghost ghost_of[k]"""
        self._keep = self._keep + (ghost_of,)
        self._check(self._lib.ani_comm_set_ghost_order(self._h, ghost_of.data_ptr() if ghost_of is not None else None))

    def forward(self, d_x, nlocal: int, stream=None):
        self._check(self._lib.ani_comm_forward(self._h, d_x, nlocal, stream))

    def reverse(self, d_f, nlocal: int, stream=None):
        self._check(self._lib.ani_comm_reverse(self._h, d_f, nlocal, stream))

    def reverse_send(self, d_f, nlocal: int, stream=None):
        self._check(self._lib.ani_comm_reverse_send(self._h, d_f, nlocal, stream))

    def reverse_unpack(self, d_f, stream=None):
        self._check(self._lib.ani_comm_reverse_unpack(self._h, d_f, stream))

    def allreduce(self, d_buf, n: int, op: str = "sum", stream=None):
        self._check(self._lib.ani_comm_allreduce_f64(self._h, d_buf, n, 0 if op == "sum" else 1, stream))
