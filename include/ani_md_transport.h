/*
 * ani_md_transport.h — where an atom has been: image flags through the wrap of the timestep loop, unwrapped positions, mean-squared
 * displacements and packed trajectory frames (lammps-ani_amd/md.py: VerletRun.set_images / set_msd / set_dump).
 *
 * NOT part of the drop-in boundary (that is ani_hip.h); a companion of ani_md.h with the same conventions.  Under LAMMPS these are
 * LAMMPS' own: the `image` flags of Domain::remap, `compute msd`, `dump custom ... ix iy iz` and `dump dcd`.
 * Units: LAMMPS `real` (A, fs, g/mol).  Every pointer is device memory unless stated otherwise; `stream` is a hipStream_t (NULL: the
 * default stream); nothing synchronises.  Return 0 on success, else a hipError_t value.  Arithmetic is fp64 whatever the handle,
 * blocks have 256 threads, and there are no floating-point atomics anywhere: the same inputs give bitwise the same outputs.
 *
 * Box: len = len3 (host pointer to three doubles) when box_dev == NULL, otherwise the three doubles at box_dev in device memory (the
 *   loop passes the barostat record's ANI_MD_NPT_LEN words: the box of the moment), as ani_md_restraints_eval takes it.
 *
 * Unwrapped coordinate -- the one definition every kernel below uses:
 *   periodic dimensions (bit k of periodic_mask):   xu[i][k] = x[i][k] + (double)image[i][k] * len[k]
 *   the product and the sum are rounded separately (no fused multiply-add), so a plain fp64 reference reproduces the bits;
 *   the other dimensions:   xu[i][k] = x[i][k].   This is LAMMPS' `xu` with the box of the moment.
 */
#ifndef ANI_MD_TRANSPORT_H
#define ANI_MD_TRANSPORT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ani_md_wrap_positions (ani_md.h) that keeps count: image[n][3] int32.  x comes out bit for bit as ani_md_wrap_positions leaves it
 * (the same expression v -= floor((v - lo) / L) * L and the same two clamps), and image[i][k] += q with q that floor as an integer;
 * where the first clamp fires (v >= lo + L, set to lo) q + 1 is added, where the second fires (v < lo, set to lo) q.  Components of
 * non-periodic dimensions are left alone, x and image both.  lo3, len3: host pointers to three doubles.  n <= 0 or periodic_mask
 * == 0: returns 0 and launches nothing.
 */
int ani_md_wrap_positions_images(double* x, int* image, int n, const double* lo3, const double* len3, int periodic_mask, void* stream);

/* out[n][3] = xu */
int ani_md_unwrap(const double* x, const int* image, int n, const double* len3, const double* box_dev, int periodic_mask, double* out,
                  void* stream);

/*
 * Mean-squared displacement of up to ANI_MD_MSD_MAXGROUP groups of atoms against one stored origin (LAMMPS `compute msd`, com no and
 * com yes at once).  A group is a union of classes: the host sorts the atoms into at most ANI_MD_MSD_MAXCLASS classes, the distinct
 * membership patterns, so that overlapping groups (all / O / H) cost one pass over the atoms.
 *   x, image          the positions and image flags of the moment
 *   x0u[n][3]         the origin, unwrapped (ani_md_unwrap at the time of the origin)
 *   mass[n]           g/mol
 *   cls[n]            int32: the class of atom i in [0, nclass), or -1 for an atom in no group (any other value counts as -1)
 *   class_count[nclass] int32, class_mass[nclass]: atoms and total mass of each class
 *   group_mask[ngroup]  int32: bit c set means class c belongs to the group
 *   work              ani_md_msd_work_size(n, nclass) doubles of scratch (host function; no initialisation needed)
 * Two launches.
 *   1. per atom d = xu - x0u; per class and block of 256 atoms the partials of ten sums, each a block sum in the fixed order of
 *      ani_md.h's sums (xor butterflies inside a wave, the four waves in order):  S2_k = sum d_k^2,  S1_k = sum d_k,
 *      Sm_k = sum m d_k  (k = x, y, z), and the number of atoms whose d has a non-finite component.
 *   2. one workgroup sums the partials in the fixed strided order of ani_md_nh_chain (per-thread accumulators over partials
 *      t, t + 256, ..., then the block sum), adds the classes of each group in ascending class order, and writes
 *      out[ngroup][ANI_MD_MSD_NOUT], indexed by the ANI_MD_MSD_* enum below, with N the group's atoms and M its mass:
 *        MSD   [4]  S2_x / N, S2_y / N, S2_z / N and their sum                                     (`compute msd`, com no)
 *        COM   [4]  the same with the group's centre-of-mass displacement removed: with dcm_k = Sm_k / M the component is
 *                   S2_k / N - 2 dcm_k S1_k / N + dcm_k^2, the fourth word their sum                 (com yes)
 *        DCM   [3]  dcm
 *        NONFINITE  atoms of the group whose d is not finite; their NaN reaches the sums, it is not masked.
 *      A group without atoms (N == 0) writes zeros.
 *   series_row != NULL: the row  step, out[0 .. ngroup * ANI_MD_MSD_NOUT)  is written there as well (1 + ngroup * ANI_MD_MSD_NOUT
 *   doubles: the host chooses the row, there is no device counter).
 * nclass outside 1..ANI_MD_MSD_MAXCLASS, ngroup outside 1..ANI_MD_MSD_MAXGROUP or n <= 0: hipErrorInvalidValue.
 */
#define ANI_MD_MSD_MAXCLASS 16
#define ANI_MD_MSD_MAXGROUP 8
#define ANI_MD_MSD_NOUT 12
enum { ANI_MD_MSD_MSD = 0, ANI_MD_MSD_COM = 4, ANI_MD_MSD_DCM = 8, ANI_MD_MSD_NONFINITE = 11 };
int ani_md_msd_work_size(int nlocal, int nclass);
int ani_md_msd_sample(const double* x, const int* image, const double* x0u, const double* mass, const int* cls, int n, int nclass,
                      const int* class_count, const double* class_mass, const int* group_mask, int ngroup, const double* len3,
                      const double* box_dev, int periodic_mask, double* work, double* out, double step, double* series_row,
                      void* stream);

/*
 * One trajectory frame in the order a DCD file holds it.  One launch.
 *   row[n]   int32: where atom i goes in the frame (the loop passes its rank by global tag); an entry outside [0, n) is skipped,
 *            never followed
 *   xyz      [3][n] fp32: all x, then all y, then all z;  xyz[k][row[i]] = (float)(unwrap ? xu[i][k] : x[i][k]), one conversion from
 *            the fp64 value, round to nearest.  image may be NULL when unwrap == 0.
 *   cell     6 doubles: lo, then len, of the box of the moment: lo from lo_dev (device, three doubles) when it is given, else from
 *            lo3 (host); len from box_dev or len3 as above.
 */
int ani_md_frame_pack(const double* x, const int* image, int n, const int* row, const double* lo3, const double* len3,
                      const double* lo_dev, const double* box_dev, int periodic_mask, int unwrap, float* xyz, double* cell,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ANI_MD_TRANSPORT_H */
