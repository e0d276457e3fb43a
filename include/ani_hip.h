/*
 * ani_hip.h — C ABI of libani_hip.so, the MI355X (gfx950) implementation of the lammps-ani hot path.
 *
 * This is the drop-in boundary: it replaces the reference's libtorch shim `class ANI`
 * (src/ani_csrc/ani.h:11-85, src/ani_csrc/ani.cpp) and everything beneath it (TorchScript LammpsANI wrapper,
 * torchani cuaev/pyaev, BmmEnsemble).  Plain pointers and sizes only; no C++ or torch types cross it; no
 * exceptions cross it (nonzero return + ani_last_error()).  The LAMMPS-side adapter
 * (lammps-ani_amd/csrc/pair_ani.cpp) and the python binding (lammps-ani_amd/ani_hip.py) both sit on this header.
 *
 * Units at the boundary are the reference's (src/ani_csrc/ani.cpp:246-262): energies kcal/mol, forces
 * kcal/mol/Angstrom, virial kcal/mol, coordinates Angstrom.
 *
 * There is NO cpu device in this library: local_rank < 0 (the reference's `device cpu`) is refused with an
 * error, and nothing here falls back to host arithmetic.
 */
#ifndef ANI_HIP_H
#define ANI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ani_handle ani_handle;

/* src/ani_csrc/ani.h:9 */
#define ANI_HARTREE2KCALMOL 627.5094738898777

/* return codes */
#define ANI_OK 0
#define ANI_ERR_ARG 1      /* bad argument / unsupported option */
#define ANI_ERR_MODEL 2    /* model file unreadable or malformed */
#define ANI_ERR_DEVICE 3   /* HIP runtime error, no device */
#define ANI_ERR_CAPACITY 4 /* a per-atom neighbour count exceeded the kernels' LDS capacity */

/*
 * Replaces ANI::ANI(model_file, local_rank, use_num_models, use_cuaev, use_fullnbr, use_single)
 * (src/ani_csrc/ani.h:31-36, src/ani_csrc/ani.cpp:35-97).
 *   model_file      flat model file (lammps-ani_amd/model_file.py), not a TorchScript archive; an optional trailing block
 *                   carries the tables of the pairwise repulsion the reference attaches to reactive models
 *                   (models/ani_models.py:50-53), which is then added to energy, forces and virial.  With use_single the
 *                   term is folded into the fast AEV backward kernel when at most 8 species are present and the block's
 *                   cutoff does not exceed Rcr (or use_cuaev = 0, where every list entry stays live); otherwise a
 *                   stand-alone kernel adds it over the whole list (ani_last_repulsion_kernel names the one that ran)
 *   local_rank      HIP device ordinal (the reference maps node-local rank % device count, src/pair_ani.cpp:255-283);
 *                   -1 = cpu is refused
 *   use_num_models  first n ensemble members, -1 = all (models/lammps_ani.py:332-343)
 *   use_cuaev       1: radial terms screened at Rcr (cuaev behaviour); 0: "pyaev" behaviour, every list pair
 *                   contributes with the cosine cutoff evaluated past Rcr.
 *                   Unlike the reference (models/lammps_ani.py:151-153,211) the virial is computed in both modes.
 *   use_fullnbr     1: ani_compute_full will be used, 0: ani_compute_half
 *   use_single      1: fp32 arithmetic on device (energy/virial sums in fp64) — the fast path (MFMA, tuned AEV kernels);
 *                   0: fp64 throughout (the reference's `double`), a plain correctness path without MFMA
 * On failure *out is NULL and ani_last_error(NULL) holds the message.
 */
int ani_create(const char* model_file, int local_rank, int use_num_models, int use_cuaev, int use_fullnbr,
               int use_single, ani_handle** out);

void ani_destroy(ani_handle* h);

/* message of the last failure on this handle (or, with h == NULL, of the last failed ani_create) */
const char* ani_last_error(const ani_handle* h);

/* model.attr("num_models") / model.attr("use_num_models") (src/ani_csrc/ani.cpp:66,90) and model constants */
int ani_num_models(const ani_handle* h);
int ani_use_num_models(const ani_handle* h);
int ani_num_species(const ani_handle* h);
int ani_aev_length(const ani_handle* h);
double ani_cutoff_radial(const ani_handle* h);
double ani_cutoff_angular(const ani_handle* h);

/*
 * Replaces ANI::compute, full-neighbour-list overload (src/ani_csrc/ani.h:54-67, src/ani_csrc/ani.cpp:183-265).
 *   species[ntotal]        0-based species (LAMMPS type-1, src/pair_ani.cpp:110); read only when ago == 0
 *   coordinates[ntotal*3]  every call
 *   ilist_unique[nlocal], numneigh[nlocal], jlist[npairs]
 *                          the LAMMPS full list flattened in ilist order, neighbour indices already masked with
 *                          NEIGHMASK (src/pair_ani.cpp:129-150); read only when ago == 0 and cached on the device
 *                          otherwise (src/ani_csrc/ani.cpp:213-229).  numneigh[ii] belongs to centre ilist_unique[ii].
 *                          A LAMMPS full list is symmetric between owned atoms (j in i's list exactly when i in j's); a list
 *                          that is not is accepted and costs the symmetric radial collection (option aev_symmetric_radial).
 *   ago                    neighbor->ago: 0 = the list was rebuilt this step
 *   eflag_atom, vflag      whether out_atomic_energies / out_virial are wanted
 *   out_energy             total energy of the nlocal centres, self energies included
 *   out_force[ntotal*3]    overwritten with -dE/dx for local AND ghost atoms (the caller reverse-communicates ghosts)
 *   out_atomic_energies[nlocal]  per-centre energies in ilist order, or NULL
 *   out_virial[9]          row-major 3x3, -sym(sum dE/d(diff) x diff) (models/lammps_ani.py:199-200,215), or NULL
 */
int ani_compute_full(ani_handle* h, int ntotal, int nlocal, const int64_t* species, const double* coordinates,
                     int64_t npairs, const int* ilist_unique, const int* jlist, const int* numneigh, int ago,
                     int eflag_atom, int vflag, double* out_energy, double* out_force, double* out_atomic_energies,
                     double* out_virial);

/*
 * Replaces ANI::compute, half-neighbour-list overload (src/ani_csrc/ani.h:39-51, src/ani_csrc/ani.cpp:100-180).
 *   atom_index12[2*npairs_half]  [0:n] = i, [n:2n] = j (src/pair_ani.cpp:144-145); every atom < nlocal is a centre.
 */
int ani_compute_half(ani_handle* h, int ntotal, int nlocal, const int64_t* species, const double* coordinates,
                     int64_t npairs_half, const int64_t* atom_index12, int ago, int eflag_atom, int vflag,
                     double* out_energy, double* out_force, double* out_atomic_energies, double* out_virial);

/*
 * Device-resident variant; replaces the Kokkos tensor overload (src/ani_csrc/ani.h:70-84,
 * src/ani_csrc/ani.cpp:268-316, caller src/pair_ani_kokkos.cpp:143-191).  Every d_* pointer is device memory on the
 * handle's device; nothing is copied to the host and nothing synchronises.
 *   d_species[ntotal]   int32, read when ago == 0
 *   d_x[ntotal*3]       double positions (LAMMPS atomKK->k_x layout)
 *   d_ilist, d_numneigh, d_jlist   as above, int32, read when ago == 0 (cached / re-bucketed on the device)
 *   d_f[ntotal*3]       double; forces are ADDED in place (src/pair_ani_kokkos.cpp:190-191)
 *   d_ev[10]            double; overwritten with {energy, virial[9]} (virial zero unless vflag)
 *   d_eatom[nlocal]     double per-centre energies (overwritten) or NULL
 *   stream              hipStream_t to enqueue on; NULL is the HIP default (null) stream, i.e. the caller's
 *                       own ordering domain (Kokkos' / torch's default stream), NOT a private stream
 */
int ani_compute_full_device(ani_handle* h, int ntotal, int nlocal, const int* d_species, const double* d_x,
                            int64_t npairs, const int* d_ilist, const int* d_jlist, const int* d_numneigh, int ago,
                            int eflag_atom, int vflag, double* d_f, double* d_ev, double* d_eatom, void* stream);

/*
 * Per-atom virial, for `compute stress/atom`, `compute centroid/stress/atom` and `compute heat/flux`.  Arms the NEXT step only
 * (one call of ani_compute_full / ani_compute_half, of ani_compute_full_device, or one ani_step_begin ... ani_step_finish
 * sequence), the way LAMMPS sets vflag_atom only on the steps a compute reads it; an entry point that fails still takes the arming.
 *   out     [ntotal][ncomp] doubles, indexed by atom (not in ilist order); host memory for the host entry points, device memory
 *           (the handle's device) for the device ones.  NULL disarms.
 *   ncomp   9: LAMMPS cvatom order  xx yy zz xy xz yz yx zx zy;  6: vatom  xx yy zz xy xz yz of the symmetric part.
 *           Anything else returns ANI_ERR_ARG (and leaves the handle unarmed).
 * Definition (site-energy form).  E = sum_i E_i with E_i the per-centre energy (out_atomic_energies), and
 *     W_j = sum over the centres i that have j in their list of  (x_j - x_i) (outer) F_j^(i),   F_j^(i) = -dE_i/dx_j,
 * "xy" = sum (x_j - x_i)_x F_y, in kcal/mol like out_virial.  This is the per-atom virial that makes
 * J = sum_j (e_j v_j - W_j . v_j) an exact heat current for that energy split (Fan et al., PRB 92, 094301, 2015): each term goes to
 * the atom that RECEIVES the force, the term j == i has weight 0.  Consequences: the sum of W_j over all ntotal rows is the
 * unsymmetrised global virial, its symmetric part the out_virial of the same call; ghost atoms receive terms (their rows belong to
 * their owners, like ghost force rows); the pairwise repulsion of REPULXTB models, half of the pair term per list entry, splits
 * half / half between the two atoms of a pair of centres.
 * Where the rows go follows the force array of the entry point:
 *   ani_compute_full / _half   every ntotal row is overwritten; the ghost rows hold what belongs to the ghosts and the caller
 *                              folds them into their owners (LAMMPS: reverse_comm with 9 values per atom when newton is off).
 *                              Armed with a communicator attached (ani_attach_comm): ANI_ERR_ARG -- no 9-wide reverse exchange.
 *   ani_compute_full_device    added into out like d_f (overwritten under option device_overwrite_forces), every ntotal row;
 *                              with a ghost fold installed (ani_set_ghost_fold) the ghost rows are folded into their owners'
 *                              rows and are NOT written.
 *   ani_step_begin ... finish  added / overwritten like d_f, every ntotal row (a split step applies no fold): both backward
 *                              halves add into one accumulator, ani_step_finish writes out.
 * Both precisions (per-atom accumulators in the handle's precision).  An armed step runs separate instantiations of the backward
 * kernels, with nine float atomics per scattered term; unarmed steps run exactly the kernels they ran before.
 */
int ani_request_atom_virial(ani_handle* h, double* out, int ncomp);

/*
 * Ensemble model deviation: the spread between the members of the ensemble, the trust signal of query-by-committee (torchani's
 * energies_qbcs) and of DeePMD's model_devi.  Arms the NEXT call of ani_compute_full / ani_compute_half or of
 * ani_compute_full_device only (an entry point that fails still takes the arming); all pointers NULL disarms.  Pointers are host
 * memory for the host entry points, device memory (the handle's device) for the device entry point.  Every output is
 * OVERWRITTEN.  Any pointer may be NULL (that output is not formed).
 * Definitions.  M = ani_use_num_models(h), at least 2 (else ANI_ERR_ARG, the handle stays unarmed).  E_i^m: energy of local
 * centre i under member m, self energy included (the mean over m is eatom[i]).  F_j^m = -d(sum_i E_i^m)/dx_j over the centres of
 * this call, network part only: the repulsion of REPULXTB models is the same for every member and drops out of every deviation.
 * Bars denote the mean over members.  kcal/mol and kcal/mol/A.  The normaliser is the population one, 1/M, everywhere: torchani's
 * unbiased sigma is sigma * sqrt(M / (M - 1)).
 *   member_energy   [M]               sum over local centres of E_i^m plus this call's repulsion energy; the mean over m is ev[0]
 *                                     up to rounding.  Adds across ranks: sum over ranks, then rho = std(E^m) / sqrt(N) (QBC).
 *   atom_energy_dev [nlocal]          sigma_E,i = sqrt((1/M) sum_m (E_i^m - mean E_i)^2), indexed like eatom.
 *   member_dforce   [ntotal][M][3]    dF_j^m = F_j^m - mean F_j for every row; ghost rows hold the ghost's share, which the caller
 *                                     folds into the owner like a force (dF is linear).  With a ghost fold installed
 *                                     (ani_set_ghost_fold, device entry) the ghost rows go into their owners and are NOT written.
 *   atom_force_dev  [nlocal]          d_j = sqrt((1/M) sum_m |dF_j^m|^2) AFTER the ghost rows are folded into their owners
 *                                     (DeePMD's per-atom force deviation).
 *   summary         [4]               {max d_j, min d_j, sum d_j, max sigma_E,i} over the local atoms (nlocal == 0: {0, inf, 0,
 *                                     0}); ranks reduce them with max / min / sum / max.
 * atom_force_dev and summary need folded rows: the call has no ghosts (ntotal == nlocal), or it is ani_compute_full_device with a
 * ghost fold installed (fp32).  Otherwise, and for any force output (member_dforce, atom_force_dev, summary) of a host entry point
 * with a communicator attached, the call returns ANI_ERR_ARG, naming the reason, before it enqueues any work.  ani_step_begin on an
 * armed handle returns ANI_ERR_ARG (the split step cannot return a deviation).
 * Cost.  member_energy / atom_energy_dev alone: one small kernel after the step, no extra backward pass.  Force outputs: every
 * member's own dE/dAEV rows (the fused MLP runs (tile, member) items, also under option mlp_fused 3; the per-layer and fp64 paths add
 * one product per member), then M more passes of the step's AEV backward kernel, each on dg_m = dE_m/dAEV - mean, into a scratch
 * accumulator.  Both precisions.  The step's own outputs (energy, forces, virial, eatom, an atom virial armed on the same step)
 * do not change; unarmed steps run exactly the kernels they ran before.
 */
int ani_request_model_deviation(ani_handle* h, double* member_energy, double* atom_energy_dev, double* member_dforce,
                                double* atom_force_dev, double* summary);

/*
 * Ghosts that are images of the rank's OWN atoms (one rank with periodic boundaries; the self-images of a rank whose brick spans
 * the box in some direction): their two exchanges of a step folded into the step's own first and last kernel.  With a fold
 * installed, ani_compute_full_device
 *   - computes the position of ghost g (atom nlocal + g) as d_x[d_owner[g]] + d_shift[g] and writes it to d_x as well (the
 *     forward communication: d_x is written although the prototype says const), and
 *   - adds the force rows of an atom's images into the atom's own row of d_f; the ghost rows of d_f are NOT written (the reverse
 *     communication, comm->reverse_comm(this) of src/pair_ani.cpp:197-201 for a one-rank run).
 * Every ghost must be such an image (d_owner[g] in [0, nlocal)): a mixed ghost shell keeps its exchange kernels.  The maps belong
 * to a list epoch: installed after the list (ago == 0 call or ani_build_list_device), cleared by the next one; device pointers,
 * kept, not copied.  d_owner == NULL clears.  fp32 handles only.  One host synchronisation (rebuild steps only).
 */
int ani_set_ghost_fold(ani_handle* h, const int64_t* d_owner, const double* d_shift, int nghost, void* stream);
/*
 * The same fold handed over BEFORE the list it belongs to: the next ani_build_list_device / ani_build_list installs it with the
 * list it builds (nghost must equal that list's ntotal - nlocal, otherwise it is dropped), and its check -- every owner inside
 * [0, nlocal) -- comes back behind the synchronisation the build has anyway instead of one of its own; a failed check makes the
 * build return ANI_ERR_ARG.  Nothing is enqueued by this call.  d_owner == NULL clears what was staged.
 */
int ani_stage_ghost_fold(ani_handle* h, const int64_t* d_owner, const double* d_shift, int nghost);

/*
 * The same device-resident step in three calls, cut where a domain-decomposed caller exchanges ghost data, so that
 * both exchanges can run on another stream beside the work that does not need them (the reference has no
 * counterpart: its forward / reverse communication are LAMMPS' blocking MPI swaps around PairANI::compute,
 * src/pair_ani.cpp:197-201).  At the first use after a re-neighbouring the library classes the centres: those with a
 * ghost atom (index >= nlocal) anywhere in their list, and the rest (one host synchronisation per epoch).
 *   ani_step_begin         needs the positions of the nlocal OWNED atoms only: packs them, screens the neighbour lists
 *                          and computes the AEVs of the centres without ghosts.
 *   ani_step_ghosts_ready  call when d_x[nlocal..ntotal) holds this step's ghost positions (stream-ordered after the
 *                          forward exchange): the centres with ghosts, the MLP of every centre, then the backward pass
 *                          of the centres with ghosts; when its work is done the GHOST rows of d_f are final (no other
 *                          centre touches a ghost atom) and the reverse exchange can start.
 *                          (The backward pass of the centres WITHOUT ghosts is started here as well, on a less urgent
 *                          stream of the library's own, beside the one of the centres with ghosts: both only wait for the
 *                          MLP, the ghost forces still come first, and two half-size kernels side by side end sooner
 *                          than one after the other.)
 *   ani_step_finish        waits for that pass; rows [0, nlocal) of d_f, energy, virial, per-atom energies.
 * Arguments as ani_compute_full_device with ago != 0 (the list of the epoch must be in place: ani_build_list_device or a
 * call with ago == 0).  The three calls may use different streams if the caller orders them with events; results equal
 * those of the one-call step up to the order of the fp32 force atomics.  Models or precisions without the fast kernels
 * (generic AEV shapes, `double`) run the whole step inside ani_step_ghosts_ready.
 */
int ani_step_begin(ani_handle* h, int ntotal, int nlocal, const double* d_x, int eflag_atom, int vflag, double* d_f, double* d_ev,
                   double* d_eatom, void* stream);
int ani_step_ghosts_ready(ani_handle* h, void* stream);
int ani_step_finish(ani_handle* h, void* stream);

/*
 * Device-side neighbour list: does on the device what LAMMPS core does on the host for
 * `neighbor <skin> bin` + the full-list request of src/pair_ani.cpp:219-223, and installs the result in the handle
 * as this epoch's list.  After it, call ani_compute_full_device with ago != 0 and NULL list pointers until the next
 * rebuild.
 *   d_species[ntotal], d_x[ntotal*3]   owned atoms first, then ghosts (ghosts carry the periodic images)
 *   cutneigh                           force cutoff + skin (7.1 A for the reference's inputs)
 *   lo[3], hi[3]                       host doubles: a box around the atoms (sub-domain widened by the ghost cutoff);
 *                                      atoms outside it are still handled correctly (clamped into the edge cells)
 *   out_npairs                         pairs in the list (may be NULL)
 * Centres are the atoms 0..nlocal-1 in order (ilist = identity).  Synchronises `stream` once (the pair count sizes
 * the list); list order is deterministic (by cell, then atom index).
 */
int ani_build_list_device(ani_handle* h, int ntotal, int nlocal, const int* d_species, const double* d_x, double cutneigh,
                          const double* lo, const double* hi, int64_t* out_npairs, void* stream);

/*
 * The same list build for callers that hold species and positions on the HOST (the role of LAMMPS' own neighbour
 * build for a non-Kokkos run: `pair_style ani ... devlist` of lammps-ani_amd/csrc/pair_ani.cpp requests only an
 * occasional list from LAMMPS, never builds it, and calls this at re-neighbouring steps instead of flattening and
 * uploading LAMMPS' host list).  Uploads species[ntotal] (int64, as ani_compute_full takes them) and
 * coordinates[ntotal*3], builds and installs the list.  Follow with ani_compute_full(..., ago != 0, NULL list
 * pointers).  Pairs are selected by distance only: no special-bond exclusions (ANI has no topology).
 */
int ani_build_list(ani_handle* h, int ntotal, int nlocal, const int64_t* species, const double* coordinates, double cutneigh,
                   const double* lo, const double* hi, int64_t* out_npairs);
/* device pointers of the installed list (tests): numneigh[nlocal], its exclusive scan [nlocal+1], jlist[npairs] */
int ani_debug_list(ani_handle* h, const int** d_numneigh, const int** d_nbr_off, const int** d_jlist);

/*
 * Molecule finder: which molecules are in the box, from the list the step already keeps (the reference answers this outside the
 * pair style, in a second GPU program over a dumped trajectory: examples/combustion/analyze.py -- a 2 A neighbour list, bonds by a
 * per-element-pair length, connected components, a count per sorted formula).  Works on the list installed in the handle for this
 * epoch (an ago == 0 call or ani_build_list*; dense segments or capacity rows).  Arms nothing, does not touch the step's state, may
 * be called between any two steps.
 *
 * ani_set_bond_table   cut[nspecies][nspecies]: host doubles in Angstrom indexed by the model's species (ani_species_symbol names
 *     them); symmetric; an entry <= 0 means "never bonded".  ANI_ERR_ARG when nspecies != ani_num_species(h), when the table is
 *     asymmetric, or when an entry is above the smaller of the two AEV cutoffs (the list is only guaranteed complete inside the
 *     force cutoff).  Copied to the device and kept until replaced; cut == NULL clears it.  There is no default table: the numbers
 *     are the caller's chemistry.
 * ani_find_molecules_device   every pointer is device memory on the handle's device, nothing synchronises, stream == NULL is the
 *     HIP default stream.  ANI_ERR_ARG when no list is installed, no bond table is set, ntotal / nlocal differ from the epoch's,
 *     or the handle is a half-list handle (use_fullnbr == 0).  Any output pointer may be NULL.
 * ani_find_molecules   the same with host pointers: uploads the positions (and owner), runs the device entry on the handle's
 *     stream, downloads and synchronises.
 *
 * Definitions.
 *   Bond      a list entry (centre i, neighbour j) with |x_j - x_i|^2 <= cut[s_i][s_j]^2, evaluated in fp64 from the doubles passed
 *             in: d_x / coordinates [ntotal*3], NOT the handle's packed fp32 positions.  The handle's precision does not matter.
 *   Owner     a ghost neighbour g >= nlocal stands for the owned atom owner[g - nlocal] (int64 [ntotal - nlocal]).  owner == NULL
 *             uses the maps of an installed ghost fold (ani_set_ghost_fold / staged) if there is one; otherwise every ghost counts
 *             as foreign.  An owner value < 0 or >= nlocal marks a foreign ghost: an atom of another rank.
 *   Molecule  a connected component of the owned atoms under bonds, ghosts replaced by their owners.  mol_of_atom[i] (int
 *             [nlocal]) is the SMALLEST owned index in i's component: the labelling is canonical, independent of scheduling.
 *   Open molecule   one with at least one bond to a foreign ghost.  Labelled like any other and counted in the summary, but left
 *             out of the formula table: a one-rank call cannot know its composition.
 *   Formula table   formula[formula_cap][S + 1] ints, S = ani_num_species(h): the count of each species, then the number of closed
 *             molecules with that composition.  The host entry sorts the rows ascending, lexicographically by composition; the
 *             device entry writes them in unspecified order.  More distinct compositions than formula_cap: the extra rows are
 *             dropped (nothing is written past formula_cap rows), summary[1] still holds the number needed, and the host entry
 *             returns ANI_ERR_CAPACITY.  Rows beyond summary[1] are not written.
 *   Summary   summary[6] (int64): molecules; distinct closed compositions; open molecules; list entries accepted as bonds
 *             (directed: a bond between two centres is met from both ends); atoms in the largest molecule; owned atoms in open
 *             molecules.
 * Six small launches (lammps-ani_amd/csrc/ani_kernels_mol.hip): a lock-free union-find over the list, a flattening pass, a tally
 * of compositions in a hash table.  No kernel waits for another lane, wave or workgroup.
 */
int ani_set_bond_table(ani_handle* h, const double* cut, int nspecies);
int ani_find_molecules_device(ani_handle* h, int ntotal, int nlocal, const double* d_x, const int64_t* d_owner, int* d_mol_of_atom,
                              int* d_formula, int formula_cap, int64_t* d_summary, void* stream);
int ani_find_molecules(ani_handle* h, int ntotal, int nlocal, const double* coordinates, const int64_t* owner, int* mol_of_atom,
                       int* formula, int formula_cap, int64_t* summary);
/* the model file's symbol of species s ("H", "C", ...; "" outside [0, ani_num_species)): valid until ani_destroy */
const char* ani_species_symbol(const ani_handle* h, int s);

/*
 * Radial distribution functions: histograms of pair distances per ordered species pair, accumulated on the device over any number
 * of frames, from the list the step already keeps (the reference's runs leave this to LAMMPS: `compute rdf` with `fix ave/time`).
 * Works on the list installed in the handle for this epoch (an ago == 0 call or ani_build_list*; dense segments or capacity rows).
 * The installed list holds every entry the caller's list or the builder's cutneigh gave it -- nothing is dropped by distance, the
 * screening to the AEV cutoffs happens per step in a buffer of its own -- so it is complete to rmax whenever it is complete to the
 * radial cutoff Rcr, which is what a step needs of it anyway.  Arms nothing, does not touch the step's state, may be called between
 * any two steps, any number of times per epoch.  The results are integers: exact, and independent of scheduling.
 *
 * ani_rdf_configure   host call at set-up time: allocates and zeroes the accumulators for npair histograms of nbins bins on
 *     [0, rmax).  pairs[npair][2]: species indices (a, b) of the model (ani_species_symbol names them); (a, b) and (b, a) are
 *     different pairs and both may be listed.  ANI_ERR_ARG, with a message that names the offender, when nbins < 1 or nbins > 4096;
 *     rmax is not a positive finite number; rmax is above the model's radial cutoff ani_cutoff_radial(h) (the list is only
 *     guaranteed complete inside the force cutoff); a species index lies outside [0, ani_num_species(h)); the same ordered pair is
 *     listed twice; the handle is a half-list handle (use_fullnbr == 0).  A refused call changes nothing.  npair == 0 or
 *     pairs == NULL clears the configuration.  Reconfiguring discards what was accumulated.  Synchronises the device.
 * ani_rdf_accumulate_device   one frame.  Every pointer is device memory on the handle's device, nothing synchronises, stream == NULL
 *     is the HIP default stream.  ANI_ERR_ARG when nothing is configured, no list is installed, ntotal / nlocal differ from the
 *     epoch's, d_x is NULL, or the handle is a half-list handle; a refused call accumulates nothing.  nlocal == 0 is a valid frame
 *     that adds no counts.
 * ani_rdf_accumulate   the same with host positions: uploads them, runs the device entry on the handle's stream and synchronises.
 * ani_rdf_read   waits for all work on the device (the device entry runs on the caller's streams), then copies the accumulators
 *     out: counts[npair][nbins], centres[npair], frames[1], all uint64; any pointer may be NULL, nothing is written past these
 *     sizes.  reset != 0 zeroes counts, centres and frames after the copy and keeps the configuration.  ANI_ERR_ARG when nothing is
 *     configured.
 *
 * Definitions.  x: the doubles passed in (d_x / coordinates [ntotal*3]), NOT the handle's packed fp32 positions; the handle's
 * precision does not matter.  s: the species the handle keeps for the owned and ghost atoms of the epoch.
 *   Centre    ii in [0, nlocal) with i = ilist[ii] in [0, nlocal): an owned atom.  Ghosts are never centres, so with several ranks
 *             every ordered pair (owned centre, neighbour) is counted by exactly one rank and the ranks' words add up.
 *   Count     an entry j of centre i's list segment with j in [0, ntotal) (others are skipped), pair p = (s_i, s_j) configured,
 *             r = sqrt(dx*dx + dy*dy + dz*dz) in fp64 with d = x_j - x_i, and r < rmax.  A ghost neighbour counts like any other;
 *             an atom's own periodic image is a legitimate neighbour.  The list decides what is a pair: an entry listed twice
 *             counts twice, a pair the list does not hold is not counted.
 *   Bin       k = (int)(r * inv_dr), truncation of the fp64 product, with inv_dr = (double)nbins / rmax computed once; the entry
 *             adds 1 to counts[p][k] when k < nbins (r * inv_dr can round up to nbins just below rmax: such an entry is dropped).
 *             Bin k covers [k * rmax / nbins, (k + 1) * rmax / nbins).
 *   Centres   centres[p] grows per frame by the number of centres with s_i == a_p, whether or not they have neighbours.
 *   Frame     every accepted ani_rdf_accumulate* call adds 1 to frames.
 * One launch per frame (lammps-ani_amd/csrc/ani_kernels_rdf.hip): sixteen lanes per centre, a workgroup-private histogram of
 * 32-bit counters in 32 KiB of static LDS flushed once per workgroup into the 64-bit words with integer atomics; above
 * 8192 bins in all (npair * nbins) the kernel counts straight into the 64-bit words.  Integer atomics only; no lane, wave or
 * workgroup waits for another.  Options "rdf_lanes" (16, default, or 64: a wave per centre) and "rdf_lds" (default 1; 0 counts
 * straight into global memory at any size) exist for measurements; the results do not depend on them.
 */
int ani_rdf_configure(ani_handle* h, int nbins, double rmax, const int* pairs /* [npair][2] species a, b */, int npair);
int ani_rdf_accumulate_device(ani_handle* h, int ntotal, int nlocal, const double* d_x, void* stream);
int ani_rdf_accumulate(ani_handle* h, int ntotal, int nlocal, const double* coordinates);
int ani_rdf_read(ani_handle* h, uint64_t* counts /* [npair][nbins] */, uint64_t* centres /* [npair] */, uint64_t* frames, int reset);

/*
 * Ghost forces over RCCL instead of the caller's host MPI (the reference: comm->reverse_comm(this) after the D2H copy,
 * src/pair_ani.cpp:197-201,461-484).  With a communicator of include/ani_comm.h attached (maps of the epoch installed by the
 * caller: ani_comm_set_epoch, and ani_comm_set_ghost_order when the ghost block is in LAMMPS' swap order), the host-pointer
 * entry points ani_compute_full / ani_compute_half sum every ghost's force into its owner ON THE DEVICE before the forces
 * leave it: out_force[0 .. 3 nlocal) is then complete, the ghost rows come back as zeros, and the caller skips its reverse
 * communication.  `comm` is an `ani_comm*` (NULL detaches); not owned by the handle.
 */
int ani_attach_comm(ani_handle* h, void* comm);

/* last-step diagnostics for tests / roofline accounting (device pointers valid until the next compute or destroy) */
typedef struct {
  int nlocal, ntotal, nrows;       /* nrows: species-bucketed AEV rows incl. padding */
  int64_t npairs;                  /* list pairs cached on the device */
  const float* d_aev;              /* [nrows][aev_length] */
  const float* d_gaev;             /* [nrows][aev_length]  dE/dAEV (Hartree) */
  const int* d_row_of_centre;      /* [nlocal] row of centre ii */
  int species_count[16];           /* centres per species */
  int aev_stride;                  /* floats per row of d_aev / d_gaev */
  int aev_active_length;           /* columns in use: the AEV entries of the species present in the system */
  int error_flags;                 /* every bit the device error word has shown so far (latched at host reads and at each
                                      re-neighbouring): 1 = LDS neighbour capacity exceeded, 2 = a wait inside the
                                      one-launch MLP kernel timed out, 8 = a caller's list was not symmetric between owned
                                      atoms (informational: option aev_symmetric_radial was off for that epoch).  The device entry points cannot return these (nothing
                                      synchronises; the energy becomes NaN): a loop that finds a NaN energy reads this */
} ani_debug_view;
/*
 * Page-lock / release a caller's host array (hipHostRegister / hipHostUnregister), so that the per-step copies of the host
 * entry points from and to it are direct DMA transfers instead of the runtime's staged pageable copies (the reference copies
 * pageable every step, src/ani_csrc/ani.cpp:206-209,250-251).  Explicit, not automatic: a registration belongs to an ADDRESS
 * RANGE, and a range that is freed while registered and handed out again by the allocator would be transferred from stale
 * pages -- release before the memory is freed or reallocated.  The LAMMPS adapter registers its own out_force buffer and, per
 * neighbour-list epoch, the atom->x block (csrc/pair_ani.cpp).  Return ANI_ERR_DEVICE when the runtime refuses (overlap with
 * another registration, limits): the copies then stay pageable, nothing else changes.
 */
int ani_host_register(const void* p, size_t bytes);
int ani_host_unregister(const void* p);

/* name of the kernel that ran the MLP of the last step ("mlp_fused<3>", "mlp_chain", "mlp_pipeline", "gemm_grouped ..."): what a
 * profile's kernel statistics list it under (bench.py's roofline block names it) */
const char* ani_last_mlp_kernel(const ani_handle* h);
/* name of the kernel that added the pairwise repulsion of the last step: "aev_backward_fast" (folded into the fast AEV backward
 * kernel), "repulsion_kernel<float>" or "repulsion_kernel<double>" (the stand-alone kernel of either precision); "" for a model
 * without the block and before the first step */
const char* ani_last_repulsion_kernel(const ani_handle* h);
int ani_debug_get(ani_handle* h, ani_debug_view* out);
/* out[c], c < aev_active_length: column of the model's full AEV that column c of d_aev holds */
int ani_debug_colmap(ani_handle* h, int* out);
/* The handle's AEV stream tables (option "aev_stream_tables"), as they stand for the species present in the current epoch.
 * species == 0: none (three or more species present, a model shape off the fast kernels, fp64).  Tuple index: one species: n;
 * two: n0 (bound + 1) + n1, n_s = the centre's neighbours of (compact) species s inside Rca, each <= bound.  A descriptor is four
 * ints {first word, stream length in slots, buckets, words reserved}; a tuple's words are words[first word + slot]:
 *   backward: ia of the band's even row | ib << 8 | column position << 16 | bucket << 24 | triangular << 29 |
 *             even row valid << 30 | odd row valid << 31          (ia, ib: positions in the centre's angular list)
 *   forward:  ia | ib << 8 | bucket << 16 | valid << 24
 * Any of the four output pointers may be NULL; the others receive 4 * tuples ints / words_bwd / words_fwd words. */
typedef struct ani_stream_tables_view {
  int32_t species, bound, tuples;
  int32_t builds;        /* how often this handle has built tables (once per set of species present, not per neighbour list) */
  int64_t words_bwd, words_fwd;
  const void *d_words_bwd, *d_words_fwd;   /* device addresses, for identity checks */
  double build_ms;       /* host time of the last build */
} ani_stream_tables_view;
int ani_debug_stream_tables(ani_handle* h, ani_stream_tables_view* view, int32_t* desc_bwd, uint32_t* words_bwd, int32_t* desc_fwd,
                            uint32_t* words_fwd);
/* the last force-armed model-deviation step's dg_m = dE_m/dAEV - mean (Hartree): member m's rows at d_parts + m * member_stride
 * elements, rows and columns laid out like d_gaev; float on an fp32 handle, double on an fp64 one (valid until the next step) */
int ani_debug_deviation_parts(ani_handle* h, const void** d_parts, int64_t* member_stride);

/*
 * Options (take effect at the next call with ago == 0):
 *   "prune_absent_species" (default 1): AEV entries of species that occur nowhere in the system (neither as centre
 *       nor as neighbour) are identically zero; with 1 the kernels work on the remaining columns only (ANI-2x water:
 *       128 of 1008) and the first-layer products use the matching weight columns — the same sums without the zero
 *       terms.  0 forces the full 1008-column layout.
 *   "mlp_fused" (default 1): networks of three hidden layers (every ANI-1x / ANI-2x member) run as ONE launch in which a
 *       workgroup takes a 128-row tile through all six products of every member with the activations in registers
 *       (ani_kernels_mlpf.hip); HBM sees the AEV rows and the dE/dAEV rows only.  0 = the per-layer kernels below.  Needs a
 *       split arithmetic ("mlp_arith" 1 or 2).  With several ensemble members a work item is (tile, member), each
 *       member writing its own dE/dAEV rows, summed afterwards.  One member and fewer than ~16 000 atoms: the chained per-layer
 *       launch is faster and is used.  2 = the fused kernel whatever the size, 3 = the same with a tile's members one after
 *       the other in its workgroup (tests, measurements).  Takes effect at the next call.
 *   "aev_fused" (default 1): the per-step screening of the candidate lists (neighbour compaction) runs inside the forward AEV
 *     launch, each wave on the centre it is about to featurise, instead of as a kernel of its own in front of it; 0 = two
 *     kernels.  Same results; candidate lists longer than 256 entries and AEV shapes off the fast path take the two kernels
 *     whatever the option says.
 *   "out_force_accumulate" (default 0; the LAMMPS adapter turns it on where it adds out_force to atom->f as it is): ani_compute_full
 *     / ani_compute_half ADD the forces into out_force instead of overwriting it -- rows [0, nlocal) with a communicator attached
 *     (the ghost rows have gone home on the device), all ntotal rows otherwise -- through a page-locked buffer of the library, in
 *     chunks, the additions of one chunk running beside the copy of the next.  Nothing is added on a call that returns an error.
 *   "nbr_sorted_rows" (default 1): ani_build_list* searches the cells and groups every centre's neighbours by species in ONE kernel,
 *     into rows of a capacity taken from the longest list of the build before (a build that overflows its rows, and the first one
 *     of a handle, counts and fills dense segments instead); ani_debug_list then returns row offsets i * capacity.  0 = separate
 *     search and grouping kernels.  "nbr_onepass" 0 = always count first, then fill.  "nbr_half_cells" (default 0): cells of half
 *     the cutoff, 5 x 5 x 5 of them searched.  The same neighbour sets in every case.
 *   "mlp_fused_halves" (default 1; sixteen-row kernel): the static schedule of the fused launch may run an item as two HALF items (the
 *     lower half of a workgroup's waves takes 64 of the 128 rows, the upper half only its share of the loads; ~0.7 of the item's
 *     time each) where that shortens the launch -- the items beyond the last full round of workgroups otherwise make a round of
 *     their own with most of the chip idle.  A split the cost model likes is timed against the whole items (three launches each,
 *     once per set of tile counts, on the step that builds the schedule) and kept only if faster; results do not depend on the
 *     choice.  0 = whole items only, 2 = every item as two halves (tests, measurements).
 *   "reuse_build_list_upload" (default 0; the LAMMPS adapter turns it on): the ani_compute_full call that follows an
 *     ani_build_list with the SAME coordinates pointer uses the positions that call uploaded instead of uploading them again.
 *     For callers whose array has not changed in between (the same timestep); a caller that might hand over another array at a
 *     recycled address leaves it off.
 *   "aev_symmetric_radial" (default 1): in the backward pass a centre takes both radial terms of a pair with a neighbour that is
 *     a centre of the same call on itself (the neighbour's term read from the neighbour's dE/dAEV row) and scatters no radial
 *     gradient to it -- two thirds of the pass's global atomics; ghost neighbours keep the scatter.  0 = scatter every radial
 *     gradient.  Same results to the order of the fp32 sums.  Relies on what a LAMMPS full list guarantees (and the built-in
 *     list builder keeps): j is in i's list exactly when i is in j's.  A list handed in by the caller (ani_compute_full,
 *     ani_compute_half, ani_compute_full_device at ago == 0) is CHECKED for this once per epoch (a hash sum over the entries
 *     between owned atoms, ~0.1 ms at 100 000 atoms); an epoch whose list fails runs with the scatter of every term, sets bit 8
 *     of error_flags and says so once on stderr.  Not used by the split step (ani_step_begin ...).
 *   "aev_stream_tables" (default 1): which pair of a centre's angular neighbours a lane of the fast AEV kernels takes in a step, its
 *     block of the AEV row and its padding depend on the centre's per-species neighbour counts alone.  With 1 the lanes read this
 *     as one 32-bit word per step from tables kept per tuple of counts, built on the device when the set of species present is
 *     installed (one or two species present, either count up to 32 -- up to the angular capacity for one species; 4.2 MB / 0.9 MB of device memory, capped at 8 MiB);
 *     centres above the bound, layouts of three or more species, armed steps and the pyaev-compatible backward pass decode
 *     arithmetically as with 0.  Same pairs in the same order: AEV rows bitwise equal, forces to the order of the atomic sums.
 *     Takes effect at the next call.
 *   "aev_tickets_min" (default 40000): AEV launches over at least this many rows hand their rows to the waves by ticket (64 groups
 *     of workgroups, a counter each) instead of at a fixed stride; smaller launches keep the stride.  Same results.
 *   "mlp_fused_schedule" (default 1): which workgroup of the fused launch runs which tiles is decided on the host, once per
 *       re-neighbouring, by first-fit-decreasing on the tiles' costs (the smallest makespan that packs them into the CUs);
 *       0 = the workgroups draw tiles from a counter, costliest first.  Takes effect at the next call.
 *   "mlp_arith" (default 1): how the MLP evaluates its fp32 products; fp32 accumulation in every case, takes effect at
 *       the next call.  1, the exact split, is what the reference's "fp32 with TF32 off" means on this chip; 2 is the
 *       counterpart of its opt-in LAMMPS_ANI_ALLOW_TF32 (src/ani_csrc/ani.cpp:41-43), also selected by that variable.
 *         2 = three v_mfma_f32_32x32x16_f16 products of two-term fp16 splits: every operand, scaled by a power of two
 *             (weights so that a layer's largest sits below 2^13, activations by 2^4, gradients by 2^12; undone exactly on
 *             the accumulators), is h + l with two fp16 numbers rounded to nearest -- good to 2^-22 relative (fp32: 2^-24)
 *             for magnitudes within 2^16 of the tensor's range, 2^-25 / scale absolute below -- and the dropped l*l term is
 *             below 2^-22 of the product.  Against the fp64 oracle the forces are as close as with 1 or 0 (the error
 *             of the step is the AEV's fp32 arithmetic; bench.py "parity", tests/test_hip_properties.py).  An activation
 *             beyond 4094 or a gradient beyond 16 Hartree per unit overflows fp16: inf, NaN energy, reported -- not wrong.
 *         1 = six v_mfma_f32_32x32x16_bf16 products of the EXACT three-term bf16 splits (8+8+8 mantissa bits) of both
 *             operands; the three dropped terms are below 2^-23 of the product: one fp32 rounding.
 *         0 = the fp32-input instruction v_mfma_f32_32x32x2_f32 (1/16 of the 16-bit matrix rate on gfx950).
 *   "mlp_split_bf16": earlier name; 1 selects "mlp_arith" 1, 0 selects "mlp_arith" 0.
 *   "mlp_pipeline" (default 0: an experiment; per-layer kernels only): 1 = with one ensemble member, arithmetic 2, layers no wider than
 *       256 and more 64-row tiles than one round of chained workgroups (about 32 000 water atoms) the six MLP products run as ONE
 *       launch of persistent workgroups that walk (layer, tile) items in order, each waiting for the flag of the same rows' item
 *       of the layer before; 2 = at any size, 0 = never.  Not a default for anything since round 4: one run of the test suite in
 *       three returned a stale tile at 60 000 atoms (a read across XCDs inside a launch).  Takes effect at the next call.
 *   "mlp_chain" (default 1; per-layer kernels only): with one ensemble member and few row tiles (small systems) the six MLP products run as one
 *       chained launch instead of six grouped ones; 2 = at any size (measurement knob), 0 = never.  Takes effect at the
 *       next call.
 *   "device_overwrite_forces" (default 0): ani_compute_full_device ADDS forces into d_f like the reference's Kokkos
 *       overload (src/pair_ani_kokkos.cpp:190-191); 1 makes it overwrite d_f[0 .. 3*ntotal) instead, for callers that
 *       would otherwise clear the array first.  Takes effect at the next call.
 *   "profiling" (default 0): the reference's LAMMPS_ANI_PROFILING (src/pair_ani.cpp:49-50, src/pair_ani_kokkos.cpp:68-70,
 *       210-212): ani_compute_full_device synchronises its stream before it returns, so the caller's host timers
 *       (LAMMPS' timing breakdown) charge the device work to the pair style.  The host-pointer entry points always
 *       synchronise.  Takes effect at the next call.
 *   "full_radial_capacity" (default 0): with the radial screen at Rcr (use_cuaev = 1) the kernels reserve LDS for 3/4
 *       of the longest neighbour list (>= 128 entries) per centre -- a uniform 7.1 A list holds 37 % of its entries
 *       inside 5.1 A -- instead of all of it; a centre that needs more raises ANI_ERR_CAPACITY.  1 reserves the full
 *       list length (takes effect at the next call).
 */
int ani_set_option(ani_handle* h, const char* name, int value);
/*
 * Profiler timeline markers (rocprofv3 --marker-trace; roctx underneath).  The library brackets its own phases ("ani:
 * neighbour compaction", "ani: AEV forward", "ani: MLP forward + backward", "ani: AEV backward + finish") and marks
 * "neighbor list rebuilt" like the reference (NVTX: src/ani_csrc/ani.cpp:128,215); the adapter uses these three to
 * bracket its own work, e.g. "reverse_comm" (src/pair_ani.cpp:198-200), without a tracing dependency of its own.
 */
void ani_trace_push(const char* name);
void ani_trace_pop(void);
void ani_trace_mark(const char* name);

/* development probe: per-phase cycle counters of a diagnostic (-DABLF_STAMPS) build of the fused MLP kernel
 * (tools/mlpf_stamps.py); returns 0 and writes nothing in the shipped build */
int ani_debug_fused_stamps(unsigned long long* out16, int reset);

/* development probe (host arithmetic only, no device): the static schedule the fused MLP launch uses ("mlp_fused_schedule") for
 * ntypes kinds of work items -- count[j] items of relative cost[j], numbered type after type -- on `bins` workgroups:
 * items_out[sum count] = item numbers, workgroup after workgroup; off_out[bins + 1]; *makespan_out = the largest workgroup load */
int ani_debug_fused_schedule(int ntypes, const int* count, const double* cost, int bins, int* items_out, int* off_out,
                             double* makespan_out);
/* the same with HALF items ("mlp_fused_halves"; the sixteen-row kernel runs item sum(count) + 2 i + h as half h of item i, at half_ratio
 * of its cost): split_mode 0 none, 1 searched, 2 every item; split_out[ntypes] = how many of each type's LAST items were cut,
 * items_out[2 sum(count)] (capacity), *n_items_out = entries written, *makespan_out = the bound the packing was made for */
int ani_debug_fused_schedule_halves(int ntypes, const int* count, const double* cost, double half_ratio, int bins, int split_mode,
                                    int* split_out, int* items_out, int* off_out, int* n_items_out, double* makespan_out);

/* copy `bytes` from a device pointer of the view to host memory (synchronises the handle's stream first) */
int ani_debug_read(ani_handle* h, const void* d_src, void* host_dst, uint64_t bytes);

/* kernel timing hooks for bench.py: brackets the phases of the NEXT computes with hipEvents on the compute stream;
 * ani_phase_times returns accumulated milliseconds {aev_fwd, mlp, aev_bwd, other (finish), pack + neighbour compaction}
 * and the call count.  enable: 1 = start a fresh accumulation, 0 = stop recording (what was recorded stays readable),
 * 2 = resume. */
int ani_phase_timing(ani_handle* h, int enable);
int ani_phase_times(ani_handle* h, double* ms5, int* ncalls);

#ifdef __cplusplus
}
#endif
#endif /* ANI_HIP_H */
