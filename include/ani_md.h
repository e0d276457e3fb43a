/*
 * ani_md.h — device kernels of the LAMMPS-free timestep loop (lammps-ani_amd/md.py, bench.py, tests).
 *
 * NOT part of the drop-in boundary (that is ani_hip.h).  Under LAMMPS these steps are LAMMPS' own: `fix nve`
 * (initial_integrate / final_integrate), `fix langevin` (post_force), Neighbor::check_distance, and the forward / reverse
 * ghost communication of Comm.  The stand-in loop that produces bench.py's MD rate runs them on the device; fused here so
 * that a step is five small launches around the hot path instead of a dozen tensor operations.
 * Units: LAMMPS `real` (A, fs, g/mol, kcal/mol).  Every pointer is device memory; `stream` is a hipStream_t (NULL: the
 * default stream); nothing synchronises.  Return 0 on success, else a hipError_t value.
 */
#ifndef ANI_MD_H
#define ANI_MD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* fix nve, initial_integrate:  v += dtfm[i] f ;  x += dt v  for the nlocal owned atoms (dtfm[i] = dt/2 * ftm2v / mass_i),
 * and Neighbor::check_distance folded in:  *d2max = max(*d2max, |x_i - x_built_i|^2)  (the caller zeroes *d2max when it
 * has read it).  x, v, f: [n][3]. */
int ani_md_initial_integrate(double* x, double* v, const double* f, const double* dtfm, double dt, int nlocal,
                             const double* x_built, double* d2max, void* stream);

/* fix langevin (post_force) + fix nve final_integrate:  f += g1[i] v + g2[i] r  with r uniform in [-0.5, 0.5) per
 * component (a counter-based generator keyed by seed, step and the atom's global tag: the same atom draws the same
 * numbers whatever rank owns it), skipped when langevin == 0;  then  v += dtfm[i] f. */
int ani_md_final_integrate(double* v, double* f, const double* dtfm, int nlocal, int langevin, const double* g1,
                           const double* g2, const int64_t* tag, uint64_t seed, uint64_t step, void* stream);

/* ani_md_final_integrate of the step that ends (its `step` number) followed by ani_md_initial_integrate of the step that begins, in
 * one pass: for stretches of a run in which nothing looks at the full-step velocities between two steps.  Same arithmetic, same
 * rounding as the two calls. */
int ani_md_final_initial_integrate(double* x, double* v, double* f, const double* dtfm, double dt, int nlocal, int langevin,
                                   const double* g1, const double* g2, const int64_t* tag, uint64_t seed, uint64_t step,
                                   const double* x_built, double* d2max, void* stream);

/* Comm::forward_comm on one rank (periodic self-images):  x[nlocal + g] = x[owner[g]] + shift[g] */
int ani_md_forward_ghosts(double* x, const int64_t* owner, const double* shift, int nlocal, int nghost, void* stream);

/* the pair style's reverse communication on one rank:  f[owner[g]] += f[nlocal + g] */
int ani_md_reverse_ghosts(double* f, const int64_t* owner, int nlocal, int nghost, void* stream);
/* the same for a ghost block that is not in message order:  f[owner[g]] += f[nlocal + ghost_of[g]]  (ghost_of NULL: as above) */
int ani_md_reverse_ghosts_ordered(double* f, const int64_t* owner, const int64_t* ghost_of, int nlocal, int nghost, void* stream);

/* Several ranks: the two halves of the same exchanges around the all-to-all.
 * pack:    out[s] = x[owner[s]] + shift[s]   for the nsend atoms this rank sends (its message buffer, [nsend][3])
 * unpack:  f[owner[s]] += in[s]              for the nsend ghost forces that came back ([nsend][3]) */
int ani_md_pack_ghosts(const double* x, const int64_t* owner, const double* shift, int nsend, double* out, void* stream);
int ani_md_unpack_reverse(double* f, const int64_t* owner, int nsend, const double* in, void* stream);

/* rows of three doubles through an index list:  out[k] = src[idx[k]]  /  dst[idx[k]] = in[k]  (the ghost block of a caller
 * whose ghosts are not grouped by owner, brought into / out of message order: include/ani_comm.h ani_comm_set_ghost_order) */
int ani_md_gather_rows(const double* src, const int64_t* idx, int n, double* out, void* stream);
int ani_md_scatter_rows(double* dst, const int64_t* idx, int n, const double* in, void* stream);

/*
 * Re-neighbouring of the stand-in loop, natively (the reference's runs leave this to LAMMPS: Domain::pbc, Comm::borders,
 * Neighbor::decide).
 *   ani_md_wrap_positions     x[i][k] -> [lo[k], lo[k] + len[k]) for the periodic dimensions (bit k of periodic_mask)
 *   ani_md_ghost_shell_count  which owned atoms are ghosts of which (brick, image) combination: atom a belongs to combination c
 *                             when clo[c][k] <= x[a][k] < chi[c][k] for k = 0..2.  Counts per (combination, block of 256 atoms) into
 *                             blk_cnt[ncombo * nblk], their exclusive scan into blk_off (nblk = ceil(n / 256), at least 1), and
 *                             out_counts[0] = all hits, out_counts[1 + c] = hits of combination c (device; the caller reads them)
 *   ani_md_ghost_shell_fill   the hits themselves, combination-major, atoms ascending: send_idx[p] = atom, send_shift[p] = cshift[c]
 *   ani_md_append_ghosts      one rank: x[nlocal + g] = x[owner[g]] + shift[g], species[nlocal + g] = species[owner[g]]
 *   ani_md_check              *out = *d2max (then *d2max = 0), or +inf when ev[0] is not finite
 */
int ani_md_wrap_positions(double* x, int n, const double* lo3, const double* len3, int periodic_mask, void* stream);
int ani_md_ghost_shell_count(const double* x, int n, const double* clo, const double* chi, int ncombo, int* blk_cnt, int* blk_off,
                             int* out_counts, void* stream);
int ani_md_ghost_shell_fill(const double* x, int n, const double* clo, const double* chi, const double* cshift, int ncombo,
                            const int* blk_off, int64_t* send_idx, double* send_shift, void* stream);
int ani_md_append_ghosts(double* x, int* species, int nlocal, const int64_t* owner, const double* shift, int nghost, void* stream);
int ani_md_check(double* d2max, const double* ev, double* out, void* stream);

/*
 * FIRE energy minimisation in the loop (LAMMPS `min_style fire`; Guenole et al., Comput. Mater. Sci. 175 (2020) 109584): an
 * integrator with three global dot products and a handful of scalars, all of it on the device.  The host looks at the state
 * record only where it looks anyway (the re-neighbouring decision).
 *
 * Parameters: the defaults of LAMMPS `min_modify` are dtmax = 10 dt0, dtmin = 0.02 dt0, dtgrow 1.1, dtshrink 0.5, alpha0 0.25,
 * alphashrink 0.99, delaystep 20, initialdelay 1, halfstepback 1, dmax 0.1 A; dt0, etol, ftol and maxiter are the caller's.
 *
 * State: ANI_MD_FIRE_NSTATE doubles on the device, read by the host after a synchronisation, indexed by the ANI_MD_FIRE_* enum below:
 *   ITERATIONS done   DT   ALPHA   LAST_NEGATIVE   E_PREV   E_CUR
 *   P = sum v.f   VV = sum v.v   FF = sum f.f   (of the last iteration that was not frozen)
 *   DTV of the last move   UPHILL events   LIMITED: dmax-limited moves
 *   STOP: 0 running, 1 etol, 2 ftol, 3 maxiter, 4 non-finite energy or force norm
 *   E_FIRST and FF_FIRST: energy and ff of the start point (seen by iteration 1)   VMAX: largest |velocity component| of the last move
 *
 * ani_md_fire_init       fills the record (dt = dt0, alpha = alpha0, everything else 0) and zeroes v[nlocal][3].
 * ani_md_fire_work_size  doubles of scratch that ani_md_fire_iterate needs for nlocal atoms (no initialisation needed; the same
 *                        buffer through all iterations of a minimisation).
 * ani_md_fire_iterate    iteration k = iterations done + 1 on the nlocal owned atoms, from x, v, f = F(x) and E = ev[0] of the last
 *                        force evaluation; fm[i] = ftm2v / mass_i.  Three launches (reduce, velocity, move):
 *   1. P, vv, ff: per-block partials, then a sum over the partials, both in a fixed order -- no floating-point atomics, so the
 *      same inputs give bitwise the same sums in every launch (the branch below hangs on the sign of P).
 *   2. stop != 0: nothing at all is written -- not x, not v, not the state.  A host that looks every few iterations still finds the
 *      exact iteration and the exact point of the stop.
 *   3. stopping tests on the current point, in this order: E or ff not finite -> 4;  ff < ftol^2 -> 2;  k > 1 and
 *      (k - 1 - last_negative) > delaystep and |E - e_prev| < etol * 0.5 * (|E| + |e_prev| + 1e-8) -> 1;  iterations done == maxiter -> 3.
 *      A test that fires sets stop, records E, P, vv, ff of the point it stopped on, and ends the iteration: no move, and
 *      iterations done, dt, alpha, e_prev stay.
 *   4. P > 0:  s1 = 1 - alpha;  s2 = ff <= 1e-20 ? 0 : alpha sqrt(vv / ff);  then, if k - last_negative > delaystep:
 *      dt = min(dt dtgrow, dtmax), alpha *= alphashrink.
 *   5. P <= 0 (an uphill event, the exact zero of a start from rest included):  last_negative = k;  unless (initialdelay and
 *      k <= delaystep): alpha = alpha0 and dt *= dtshrink if that stays >= dtmin;  with halfstepback x -= 0.5 dtv_prev v, where
 *      dtv_prev is the dtv of the move before;  v = 0.
 *   6. v += dt fm[i] f;  if P > 0: v = s1 v + s2 f;  vmax = largest |component| of any v;  dtv = dt, or dmax / vmax when
 *      dtv vmax > dmax (a limited move);  x += dtv v;  *d2max = max(*d2max, |x_i - x_built_i|^2) as ani_md_initial_integrate
 *      (x_built or d2max NULL: skipped).
 *   7. iterations done = k, e_prev = e_cur = E.
 * ani_md_fire_check      ani_md_check with the state record behind it: out[0] as there, out[1 + j] = state[j]
 *                        (out: 1 + ANI_MD_FIRE_NSTATE doubles).
 */
#define ANI_MD_FIRE_NSTATE 16
enum {
  ANI_MD_FIRE_ITERATIONS = 0, ANI_MD_FIRE_DT, ANI_MD_FIRE_ALPHA, ANI_MD_FIRE_LAST_NEGATIVE, ANI_MD_FIRE_E_PREV, ANI_MD_FIRE_E_CUR,
  ANI_MD_FIRE_P, ANI_MD_FIRE_VV, ANI_MD_FIRE_FF, ANI_MD_FIRE_DTV, ANI_MD_FIRE_UPHILL, ANI_MD_FIRE_LIMITED, ANI_MD_FIRE_STOP,
  ANI_MD_FIRE_E_FIRST, ANI_MD_FIRE_FF_FIRST, ANI_MD_FIRE_VMAX
};
typedef struct ani_md_fire_params {
  double dt0, dtmax, dtmin, dtgrow, dtshrink, alpha0, alphashrink, dmax, etol, ftol;
  int delaystep, initialdelay, halfstepback, maxiter;
} ani_md_fire_params;
int ani_md_fire_work_size(int nlocal);
int ani_md_fire_init(double* state, double* v, int nlocal, const ani_md_fire_params* p, void* stream);
int ani_md_fire_iterate(double* x, double* v, const double* f, const double* fm, int nlocal, const double* ev,
                        const ani_md_fire_params* p, double* state, double* work, const double* x_built, double* d2max,
                        void* stream);
int ani_md_fire_check(double* d2max, const double* ev, const double* state, double* out, void* stream);

/*
 * Holonomic bond-length constraints in the loop, in the RATTLE form (Andersen, J. Comput. Phys. 52 (1983) 24; LAMMPS `fix shake`
 * / `fix rattle` on clusters of 2, 3 and 4 atoms): one central atom and one to three partners, every constrained bond joins the
 * centre to a partner.  Two stages per step, each one launch behind a kernel of the integrator; a loop without constraints
 * launches neither.
 *
 * Shared inputs:
 *   cl[nc][4]      int32: the centre and up to three partners as local indices (< nlocal), -1 for an unused slot; the used slots
 *                  come first, and no atom belongs to two clusters.  A wave runs one cluster size when the table is ordered by size.
 *   d[nc][3]       the bond lengths in A (slot k of d belongs to slot 1 + k of cl; unused slots are not read)
 *   w[nlocal]      any array proportional to 1 / mass_i (the loop passes its dtfm)
 *   len3, periodic_mask   as ani_md_wrap_positions (host pointer to three doubles): every bond vector is a minimum image,
 *                  minimg(a)[k] = a[k] - len3[k] rint(a[k] / len3[k]) in the periodic dimensions -- the loop wraps owned atoms at a
 *                  rebuild, so a cluster can sit across a face.
 *
 * ani_md_shake_positions   after ani_md_initial_integrate: x holds the unconstrained x', v the half-step velocity.  The old
 *   positions are rebuilt as x0 = x' - dt v (no copy is kept).  With s_k = minimg(x0_c - x0_pk) it finds g_k such that
 *       x_c = x'_c + w_c sum_k g_k s_k,   x_pk = x'_pk - w_pk g_k s_k,   | |r_k|^2 - d_k^2 | <= tol d_k^2  for every k,
 *   r_k = minimg(x_c - x_pk), by Newton on the K <= 3 unknowns from g = 0, the K x K Jacobian solved directly, at most maxiter
 *   iterations (an iteration is one solve; the test comes first, so a start that holds takes none and moves nothing).  Then
 *   v_i += (x_i - x'_i) / dt, and |x_i - x_built_i|^2 of the moved atoms is folded into *d2max as ani_md_initial_integrate does
 *   it (a workgroup maximum, then at most one integer atomic on the bit pattern; x_built or d2max NULL: skipped).
 *   v == NULL: x0 = x' and no velocity is written -- the form that projects a start configuration onto the constraints.
 *   A cluster that reaches maxiter unconverged is written with what it has, and counted.
 *
 * ani_md_rattle_velocities  after ani_md_final_integrate: with r_k = minimg(x_c - x_pk) of the current positions it finds h_k
 *   such that
 *       v_c += w_c sum_k h_k r_k,   v_pk -= w_pk h_k r_k,   r_k . (v_c - v_pk) = 0  for every k:
 *   a symmetric positive-definite K x K linear system, solved directly, no iteration.  d is not read (the constraint is on the
 *   direction of the bond as it is); the argument keeps the two stages' shared inputs in one shape.
 *
 * stats: ANI_MD_SHAKE_NSTATS `unsigned long long` words on the device, zeroed by the caller (NULL: not kept):
 *   [0] clusters that reached maxiter unconverged (accumulates over the calls)   [1] the largest iteration count
 *   [2] the largest final relative residual max_k | |r_k|^2 - d_k^2 | / d_k^2, as the bit pattern of a non-negative double
 *       (a NaN orders above every finite pattern: a blown-up cluster shows here)   [3] calls
 *   updated with integer atomics only, after a workgroup reduction.
 *
 * Both kernels: one thread per cluster, 256-thread blocks, everything in registers; no floating-point atomics anywhere, so the
 * same inputs give bitwise the same outputs; atoms in no cluster are not written.  The momentum of a cluster is conserved
 * (sum_i dx_i / w_i = 0, sum_i dv_i / w_i = 0).
 */
#define ANI_MD_SHAKE_NSTATS 4
int ani_md_shake_positions(double* x, double* v, const int* cl, const double* d, int nc, const double* w, double dt, double tol,
                           int maxiter, const double* len3, int periodic_mask, const double* x_built, double* d2max,
                           unsigned long long* stats, void* stream);
int ani_md_rattle_velocities(const double* x, double* v, const int* cl, const double* d, int nc, const double* w,
                             const double* len3, int periodic_mask, void* stream);

/*
 * Nose-Hoover chain at constant volume (LAMMPS `fix nvt`, the `temp` half of `fix npt`: Martyna, Klein, Tuckerman, J. Chem. Phys. 97
 * (1992) 2635; the explicit integrator of Martyna, Tuckerman, Tobias, Klein, Mol. Phys. 87 (1996) 1117) and the thermo record of
 * `thermo_style custom pe ke etotal temp press`.  fp64 whatever the handle.  One rank.  No floating-point atomics: every sum is
 * per-block partials (256 threads, xor butterflies inside a wave, the four waves in order), then one workgroup that strides over the
 * partials and sums its 256 accumulators in the same fixed order -- the same inputs give bitwise the same record.
 *
 * Constants: k_B = 0.0019872067 kcal/mol/K, mvv2e = 48.88821291^2, nktv2p = 68568.415 (atm).
 *
 * Chain half-step, from K2 = sum_i m_i |v_i|^2 mvv2e (twice the kinetic energy), t_target, tdof and the parameters:
 *   kt = k_B t_target, ket = tdof kt, tf = 1 / t_period, Q[0] = ket / tf^2, Q[k >= 1] = kt / tf^2 (from t_target, at every call),
 *   nf = 1 / nc_tchain, dfac = 1 - dt drag / nc_tchain, M = mtchain <= ANI_MD_NH_MAXCHAIN, eta_dot[M] read as 0.
 *     eta_dotdot[0] = (K2 - ket) / Q[0];  s = 1
 *     repeat nc_tchain times:
 *       for k = M-1 .. 1:  e = exp(-nf dt/8 eta_dot[k+1]);  eta_dot[k] = ((eta_dot[k] e + eta_dotdot[k] nf dt/4) dfac) e
 *       e = exp(-nf dt/8 eta_dot[1]);  eta_dot[0] = ((eta_dot[0] e + eta_dotdot[0] nf dt/4) dfac) e
 *       fac = exp(-nf dt/2 eta_dot[0]);  s *= fac;  K2 *= fac fac;  eta_dotdot[0] = (K2 - ket) / Q[0]
 *       eta[k] += nf dt/2 eta_dot[k]  for all k
 *       eta_dot[0] = (eta_dot[0] e + eta_dotdot[0] nf dt/4) e                                            (the same e)
 *       for k = 1 .. M-1:  e = exp(-nf dt/8 eta_dot[k+1]);  eta_dot[k] *= e;
 *                          eta_dotdot[k] = (Q[k-1] eta_dot[k-1]^2 - kt) / Q[k];  eta_dot[k] = (eta_dot[k] + eta_dotdot[k] nf dt/4) e
 *     ecouple = ket eta[0] + Q[0] eta_dot[0]^2 / 2 + sum_{k >= 1} (kt eta[k] + Q[k] eta_dot[k]^2 / 2)
 *   The caller multiplies every velocity by s.  eta_dotdot is state: the first loop of a call uses the upper links' accelerations
 *   that the call before left.
 *
 * State: ANI_MD_NH_NSTATE doubles on the device, indexed by the ANI_MD_NH_* enum below:
 *   HALF_STEPS done   K2 after the scaling   S of the last half-step   its T_TARGET   ECOUPLE   TDOF
 *   NONFINITE: calls that found K2 non-finite   ZERO   ETA, ETA_DOT, ETA_DOTDOT: ANI_MD_NH_MAXCHAIN links each (unused links stay 0)
 *   A call that finds K2 non-finite writes S = 1 (and K2 = that K2, T_TARGET, TDOF), adds one to NONFINITE and leaves HALF_STEPS,
 *   ECOUPLE and the chain.
 *
 * ani_md_nh_work_size   doubles of scratch for nlocal atoms: one partial per block of 256 atoms (host function, no device).
 * ani_md_nh_init        zeroes the record.
 * ani_md_nh_kinetic     work[b] = K2 of the owned atoms of block b (b < ceil(nlocal / 256)); mass[nlocal] in g/mol.
 * ani_md_nh_chain       one workgroup.  npart > 0: K2 = work[0] + .. + work[npart - 1] in the fixed order;  npart == 0: K2 = state[ANI_MD_NH_K2].
 *                       Then the half-step above, and the whole record is written.  params is a host pointer.
 * ani_md_nh_scale       v *= state[ANI_MD_NH_S].
 * ani_md_nh_initial_integrate   v = state[ANI_MD_NH_S] v first, then ani_md_initial_integrate.
 * ani_md_nh_final_integrate     ani_md_final_integrate without Langevin (f is not written), and in the same pass the partials of
 *                       ani_md_nh_kinetic on the new velocities into work: bit for bit what that call would write.
 *
 * ani_md_thermo: two launches (per-block partials of the six sums K_ab = sum_i m_i v_ia v_ib mvv2e in the order xx, yy, zz, xy, xz,
 * yz, then one workgroup) into out[ANI_MD_THERMO_N], indexed by the ANI_MD_THERMO_* enum below, with W_ab = ev[1 + 3 a + b] the pair
 * virial and V = volume:
 *   PE = ev[0]   KE = (K_xx + K_yy + K_zz) / 2   TEMP = 2 ke / (tdof k_B)
 *   PRESS = (K_xx + K_yy + K_zz + W_xx + W_yy + W_zz) / (3 V) nktv2p
 *   PXX PYY PZZ PXY PXZ PYZ: P_ab = (K_ab + W_ab) / V nktv2p   ETOTAL = pe + ke   ECOUPLE = nh_state[ANI_MD_NH_ECOUPLE] (0: NULL)
 *   ECONSERVE = etotal + ecouple   VOL = volume   K2 = 2 ke   ZERO
 *   with_virial == 0: PRESS .. PYZ are NaN.  work: ani_md_thermo_work_size(nlocal) doubles.
 */
#define ANI_MD_NH_NSTATE 32
#define ANI_MD_NH_MAXCHAIN 8
#define ANI_MD_THERMO_N 16
enum {
  ANI_MD_NH_HALF_STEPS = 0, ANI_MD_NH_K2, ANI_MD_NH_S, ANI_MD_NH_T_TARGET, ANI_MD_NH_ECOUPLE, ANI_MD_NH_TDOF, ANI_MD_NH_NONFINITE,
  ANI_MD_NH_ZERO, ANI_MD_NH_ETA = 8, ANI_MD_NH_ETA_DOT = 16, ANI_MD_NH_ETA_DOTDOT = 24
};
enum {
  ANI_MD_THERMO_PE = 0, ANI_MD_THERMO_KE, ANI_MD_THERMO_TEMP, ANI_MD_THERMO_PRESS, ANI_MD_THERMO_PXX, ANI_MD_THERMO_PYY,
  ANI_MD_THERMO_PZZ, ANI_MD_THERMO_PXY, ANI_MD_THERMO_PXZ, ANI_MD_THERMO_PYZ, ANI_MD_THERMO_ETOTAL, ANI_MD_THERMO_ECOUPLE,
  ANI_MD_THERMO_ECONSERVE, ANI_MD_THERMO_VOL, ANI_MD_THERMO_K2, ANI_MD_THERMO_ZERO
};
typedef struct ani_md_nh_params {
  double dt, t_period, drag;
  int mtchain, nc_tchain;
} ani_md_nh_params;
int ani_md_nh_work_size(int nlocal);
int ani_md_nh_init(double* state, void* stream);
int ani_md_nh_kinetic(const double* v, const double* mass, int nlocal, double* work, void* stream);
int ani_md_nh_chain(double* state, const double* work, int npart, double t_target, double tdof, const ani_md_nh_params* params,
                    void* stream);
int ani_md_nh_scale(double* v, int nlocal, const double* state, void* stream);
int ani_md_nh_initial_integrate(double* x, double* v, const double* f, const double* dtfm, double dt, int nlocal,
                                const double* x_built, double* d2max, const double* state, void* stream);
int ani_md_nh_final_integrate(double* v, const double* f, const double* dtfm, const double* mass, int nlocal, double* work,
                              void* stream);
int ani_md_thermo_work_size(int nlocal);
int ani_md_thermo(const double* v, const double* mass, int nlocal, const double* ev, int with_virial, double tdof, double volume,
                  const double* nh_state, double* work, double* out, void* stream);

/*
 * Isotropic Nose-Hoover barostat on top of the chain above (LAMMPS `fix npt temp ... iso ...` with `mtk yes` and pchain > 0: Martyna,
 * Tobias, Klein, J. Chem. Phys. 101 (1994) 4177; the integrator of Tuckerman et al., J. Phys. A 39 (2006) 5629).  fp64 whatever the
 * handle, one rank, no floating-point atomics, nothing synchronises.  The box lives in the barostat record on the device; the host
 * reads it where it looks anyway (ani_md_npt_check).
 *
 * Notation: N owned atoms; tdof, kt = k_B t_target, K2 as above; Wtr = (ev[1] + ev[5]) + ev[9], the pair virial of the last force
 * evaluation; V = len[0] len[1] len[2] of the record; W = ((N + 1) kt) (p_period p_period); wd the one scalar strain rate (the three
 * equal strain rates of `iso`); c the fixed point of the dilation, the box centre at ani_md_npt_init.
 *
 * Barostat chain: the chain half-step above -- the same device function -- on K2 := W wd^2 with tdof := 1 (ket = kt), t_period :=
 * p_period, drag := 0, M := mpchain, nc := nc_pchain and the barostat's own eta, eta_dot, eta_dotdot; then wd *= s.  The barostat has
 * no drag.
 * Strain-rate update:  P = (K2 + Wtr) / (3 V) nktv2p;   wd += dt/2 [ (P - p_target) V / nktv2p + K2 / (3 N) ] / W.
 *
 * First half (ani_md_npt_chain phase 0, then ani_md_npt_initial_integrate):
 *   1. barostat chain    2. thermostat chain on K2, giving s; K2 *= s^2 (the chain does it)    3. strain-rate update with that K2
 *   4. fv = exp(-dt/2 wd (1 + 1/N)),  mu = exp(dt/2 wd)
 *   5. per atom:  v = (s fv) v;  v += dtfm f;  x = c + mu (x - c);  x += dt v;  x = c + mu (x - c)
 *   6. box:  lo = c + mu^2 (lo - c),  len *= mu^2;  ratio[k] = len_new[k] / len_old[k];  omega += dt wd
 *   7. every ghost shift row *= ratio, per component (shifts are set exactly at every re-neighbouring: the rounding of this product
 *      does not accumulate beyond one list epoch)
 * Second half (ani_md_npt_final_integrate, ani_md_npt_chain phase 1, ani_md_nh_scale):
 *   1. per atom:  v += dtfm f;  v *= fv  (the fv of the record: the same wd as the first half), and the partials of K2 in the same pass
 *   2. K2 summed in the fixed order    3. strain-rate update with the new K2 and the new Wtr    4. thermostat chain, then v *= s
 *   5. barostat chain
 * This is FixNH's order for iso, mtk yes, pchain > 0.
 *
 * Conserved:  pe + ke + ecouple(thermostat, ANI_MD_NH_ECOUPLE) + ecouple(barostat, ANI_MD_NPT_ECOUPLE) with
 *   ecouple(barostat) = 3 (W wd^2 / 2 + ecouple of the barostat chain) + p_target (V - V0) / nktv2p,   V0 the volume at ani_md_npt_init.
 * The factor 3: the three equal strain rates are one scalar here.
 *
 * Barostat record: ANI_MD_NPT_NSTATE doubles on the device, indexed by the ANI_MD_NPT_* enum below:
 *   HALF_STEPS done   OMEGA_DOT = wd   OMEGA = sum dt wd   PRESS: P of the last strain-rate update   its P_TARGET   W   FV   MU
 *   LO, LEN: the box (three each)   RATIO of the last first half (three)   C (three)   V0   ECOUPLE(barostat)
 *   NONFINITE: half-steps that found K2, Wtr or the new wd non-finite   NATOMS = N   ETA, ETA_DOT, ETA_DOTDOT of the barostat chain:
 *   ANI_MD_NH_MAXCHAIN links each (unused links stay 0)   ECOUPLE_CHAIN: ecouple of the barostat chain alone   VOL = V   the rest 0
 * A half-step that finds K2, Wtr or the new wd non-finite writes S = 1 into the NH record as ani_md_nh_chain does (with K2, T_TARGET,
 * TDOF, one more in NONFINITE), fv = mu = 1 and ratio = 1 into this one, adds one to NONFINITE and leaves HALF_STEPS, the box, wd and
 * both chains.
 *
 * ani_md_npt_init       fills the record: lo, len, c = lo + len / 2, V0 = V, N, fv = mu = ratio = 1, the rest 0 (host arguments).
 * ani_md_npt_chain      one workgroup.  phase 0: steps 1-4 and 6 of the first half; phase 1: steps 2-5 of the second.  npart > 0: K2 =
 *                       the partials in the fixed order of ani_md_nh_chain; npart == 0: K2 = nh_state[ANI_MD_NH_K2].  Writes both records.
 *                       t_target and p_target (atm) are arguments: the host ramps them and reads nothing.  params: host pointer.
 * ani_md_npt_initial_integrate   step 5 on rows [0, nlocal) with the displacement fold of ani_md_initial_integrate against x_built
 *                       (which is NOT rescaled: the displacement includes the dilation), and step 7 on shift rows [0, nghost), in one
 *                       launch over nlocal + nghost rows.
 * ani_md_npt_final_integrate     step 1 of the second half; work: the partials of ani_md_nh_kinetic on the new velocities, bit for bit.
 * ani_md_npt_check      ani_md_check with the barostat record behind the word: out[1 + j] = npt_state[j]
 *                       (out: 1 + ANI_MD_NPT_NSTATE doubles).
 */
#define ANI_MD_NPT_NSTATE 56
enum {
  ANI_MD_NPT_HALF_STEPS = 0, ANI_MD_NPT_OMEGA_DOT, ANI_MD_NPT_OMEGA, ANI_MD_NPT_PRESS, ANI_MD_NPT_P_TARGET, ANI_MD_NPT_W, ANI_MD_NPT_FV,
  ANI_MD_NPT_MU, ANI_MD_NPT_LO = 8, ANI_MD_NPT_LEN = 11, ANI_MD_NPT_RATIO = 14, ANI_MD_NPT_C = 17, ANI_MD_NPT_V0 = 20, ANI_MD_NPT_ECOUPLE,
  ANI_MD_NPT_NONFINITE, ANI_MD_NPT_NATOMS, ANI_MD_NPT_ETA = 24, ANI_MD_NPT_ETA_DOT = 32, ANI_MD_NPT_ETA_DOTDOT = 40,
  ANI_MD_NPT_ECOUPLE_CHAIN = 48, ANI_MD_NPT_VOL
};
typedef struct ani_md_npt_params {
  double dt, t_period, drag, p_period;
  int mtchain, nc_tchain, mpchain, nc_pchain;
} ani_md_npt_params;
int ani_md_npt_init(double* npt_state, const double* lo3, const double* len3, int nlocal, void* stream);
int ani_md_npt_chain(int phase, double* nh_state, double* npt_state, const double* work, int npart, const double* ev, double t_target,
                     double p_target, double tdof, const ani_md_npt_params* params, void* stream);
int ani_md_npt_initial_integrate(double* x, double* v, const double* f, const double* dtfm, double dt, int nlocal,
                                 const double* x_built, double* d2max, const double* nh_state, const double* npt_state,
                                 double* shift, int nghost, void* stream);
int ani_md_npt_final_integrate(double* v, const double* f, const double* dtfm, const double* mass, int nlocal,
                               const double* npt_state, double* work, void* stream);
int ani_md_npt_check(double* d2max, const double* ev, const double* npt_state, double* out, void* stream);

/*
 * Umbrella restraints on collective variables in the loop: a harmonic bias on a distance, an angle or a torsion (PLUMED `DISTANCE` /
 * `ANGLE` / `TORSION` + `RESTRAINT`, LAMMPS `fix restrain bond` / `angle`), as two launches behind the force evaluation, and a
 * device-side series of the values (PLUMED `PRINT`).  fp64 whatever the handle, one rank, no floating-point atomics, nothing
 * synchronises.
 *
 * Tables (device):
 *   atoms[nr][4]   int32: the 2, 3 or 4 owned atoms of a restraint as local indices (< natoms), all distinct, -1 in unused slots
 *   kind[nr]       int32: ANI_MD_RESTRAINT_DISTANCE (slots a, b), _ANGLE (a, b, c; b is the apex), _TORSION (a, b, c, d)
 *   kappa[nr]      >= 0, kcal/mol/A^2 (distance) or kcal/mol/rad^2 (angle, torsion); PLUMED's KAPPA=100 kJ/mol/rad^2 is 23.9006
 *   centre[nr]     A or rad
 * Box: len = len3 (host pointer to three doubles) when box_dev == NULL, otherwise the three doubles at box_dev in device memory (the
 *   loop passes the barostat record's ANI_MD_NPT_LEN words: the box of the moment).  Every difference vector is a minimum image,
 *   minimg(a)[k] = a[k] - len[k] rint(a[k] / len[k]) in the periodic dimensions (bit k of periodic_mask).
 * Bias:  e = kappa / 2 D^2,  F_i = -kappa D dcv/dx_i,  D = cv - centre; for a torsion D is folded into (-pi, pi]:
 *   D -= 2 pi rint(D / (2 pi)), then D += 2 pi where D <= -pi.
 * Collective variables:
 *   distance  r = minimg(x_a - x_b), cv = |r|;  dcv/dx_a = r / |r|, dcv/dx_b = -r / |r|
 *   angle     u = minimg(x_a - x_b), w = minimg(x_c - x_b), c = u^ . w^ clamped to [-1, 1], cv = acos(c) in [0, pi];  with
 *             s = sqrt((1 - c) (1 + c)):  dcv/dx_a = (c u^ - w^) / (|u| s),  dcv/dx_c = (c w^ - u^) / (|w| s),  dcv/dx_b = minus their sum
 *   torsion   F = minimg(x_a - x_b), G = minimg(x_b - x_c), H = minimg(x_d - x_c), A = F x G, B = H x G,
 *             cv = atan2(-|G| F . B, A . B): the IUPAC / PLUMED sign -- a = (1,0,0), b = (0,0,0), c = (0,0,1), d = (cos t, sin t, 1)
 *             gives cv = t.  With T = (F . G) / (|A|^2 |G|) A - (H . G) / (|B|^2 |G|) B:
 *             dcv/dx_a = -|G| / |A|^2 A,  dcv/dx_d = |G| / |B|^2 B,  dcv/dx_b = -dcv/dx_a + T,  dcv/dx_c = -dcv/dx_d - T
 * Virial of a restraint:  W_ab = sum_i rho_i,a F_i,b  with rho the minimum-image positions relative to slot b: distance r, 0; angle
 *   u, 0, w; torsion F, 0, -G, H - G.  Nine entries in ev's order, W_ab at 3 a + b.
 * A restraint whose D or gradient is not finite (a collinear torsion, an angle at 0 or pi, coincident atoms; also a table entry
 *   that names an atom outside [0, natoms) or an unknown kind, which reads no position) writes e = NaN with zero forces and zero
 *   virial, and is counted: the NaN reaches ev[0], where the loop's look finds it.
 *
 * ani_md_restraints_eval    one thread per restraint, 256-thread blocks, registers only.  Writes cv[nr], e[nr], the slot forces
 *   fslot[nr][4][3] (zeros in unused slots) and w[nr][9], and nothing else: restraints may share atoms.
 * ani_md_restraints_apply   reads the host-built gather table in CSR form: touched[ntouched] the atoms in any restraint, ascending;
 *   row_ptr[ntouched + 1]; entries[row_ptr[t] .. row_ptr[t + 1]) the words 4 restraint + slot of atom touched[t], ascending.  One
 *   thread per touched atom sums its entries' slot forces in table order into an accumulator that starts from 0, then f[i] += the
 *   accumulator; rows of atoms in no restraint are not written.  One further workgroup of the same launch sums e and w in the fixed
 *   order of the chain's sums (per-thread strided accumulators, then the block sum), then  ev[0] += E;  with_virial != 0:
 *   ev[1..10) += W, otherwise those words are not touched;  and writes the record and, with series_row != NULL, the row
 *   step, cv[0..nr), e[0..nr)  at series_row (1 + 2 nr doubles: the host chooses the row, there is no device counter).
 *   The same inputs give bitwise the same f, ev and record.
 *   A word of the table that points outside -- touched[t] outside [0, natoms), an entry outside [0, 4 nr) -- is skipped (an atom
 *   with all its entries, or the one entry), never followed, and the sums' workgroup counts such words: any of them makes E NaN
 *   (ev[0] and the record's EBIAS) like a non-finite restraint, so a table that drops force cannot pass for a good one.  row_ptr is
 *   trusted: ascending, within entries.
 * Record: ANI_MD_RESTRAINT_NREC doubles on the device, zeroed by the caller at the start, indexed by the ANI_MD_RESTRAINT_REC_* enum:
 *   EVALUATIONS (one more per apply)   EBIAS = E   VIRIAL = W (nine)   NONFINITE restraints of this evaluation
 *   MAX_DELTA: the largest |D| among the finite ones   SKIPPED words of the gather table   ZERO (two)
 * No alignment beyond that of the element types is asked of any pointer.
 * nr <= 0: both return 0 and launch nothing.
 */
#define ANI_MD_RESTRAINT_NREC 16
#define ANI_MD_RESTRAINT_DISTANCE 0
#define ANI_MD_RESTRAINT_ANGLE 1
#define ANI_MD_RESTRAINT_TORSION 2
enum {
  ANI_MD_RESTRAINT_REC_EVALUATIONS = 0, ANI_MD_RESTRAINT_REC_EBIAS, ANI_MD_RESTRAINT_REC_VIRIAL, ANI_MD_RESTRAINT_REC_NONFINITE = 11,
  ANI_MD_RESTRAINT_REC_MAX_DELTA, ANI_MD_RESTRAINT_REC_SKIPPED, ANI_MD_RESTRAINT_REC_ZERO
};
int ani_md_restraints_eval(const double* x, int natoms, const int* atoms, const int* kind, const double* kappa, const double* centre,
                           int nr, const double* len3, const double* box_dev, int periodic_mask, double* cv, double* e, double* fslot,
                           double* w, void* stream);
int ani_md_restraints_apply(double* f, int natoms, double* ev, int with_virial, const int* touched, const int* row_ptr,
                            const int* entries, int ntouched, const double* fslot, const double* cv, const double* e, const double* w,
                            const double* centre, const int* kind, int nr, double* record, double step, double* series_row,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ANI_MD_H */
