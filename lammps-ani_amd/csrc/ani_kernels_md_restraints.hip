// ani_kernels_md_restraints.hip — umbrella restraints on collective variables in the timestep loop (include/ani_md.h,
// ani_md_restraints_eval / ani_md_restraints_apply)
#include "ani_md_device.h"

namespace {

// ---- umbrella restraints on collective variables (include/ani_md.h, ani_md_restraints_eval / ani_md_restraints_apply) --------
// Two launches behind the force evaluation.  eval: one thread per restraint, everything in registers, writes only its own rows of
// cv, e, fslot and w -- restraints share atoms, so nothing is added into f here.  apply: one thread per touched atom walks the
// host-built gather table in its fixed order (no floating-point atomics), and one further workgroup sums e and w in the fixed
// order of the sums above and writes ev, the record and the series row.
static_assert(ANI_MD_RESTRAINT_REC_ZERO + 2 == ANI_MD_RESTRAINT_NREC, "the apply kernel writes the whole record");

__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
// cv - centre, for a torsion folded into (-pi, pi]
__device__ __forceinline__ double restraint_delta(double cv, double centre, int kd) {
  double d = cv - centre;
  if (kd == ANI_MD_RESTRAINT_TORSION) {
    const double twopi = 6.283185307179586, pi = 3.141592653589793;
    d -= twopi * rint(d / twopi);
    if (d <= -pi) d += twopi;
  }
  return d;
}

__global__ __launch_bounds__(256) void restraints_eval_kernel(const double* __restrict__ x, int natoms, const int* __restrict__ atoms,
                                                              const int* __restrict__ kind, const double* __restrict__ kappa,
                                                              const double* __restrict__ centre, int nr, double L0, double L1, double L2,
                                                              const double* __restrict__ box_dev, int pmask, double* __restrict__ cv_out,
                                                              double* __restrict__ e_out, double* __restrict__ fslot,
                                                              double* __restrict__ w_out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= nr) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double L[3] = {L0, L1, L2};
  if (box_dev) { L[0] = box_dev[0]; L[1] = box_dev[1]; L[2] = box_dev[2]; }
  const int a[4] = {atoms[4 * (size_t)r], atoms[4 * (size_t)r + 1], atoms[4 * (size_t)r + 2], atoms[4 * (size_t)r + 3]};
  const int kd = kind[r];
  const int na = kd == ANI_MD_RESTRAINT_DISTANCE ? 2 : kd == ANI_MD_RESTRAINT_ANGLE ? 3 : 4;
  // a table that names an atom outside [0, natoms) or an unknown kind reads nothing and ends as a non-finite restraint
  bool ok = kd >= ANI_MD_RESTRAINT_DISTANCE && kd <= ANI_MD_RESTRAINT_TORSION;
#pragma unroll
  for (int m = 0; m < 4; m++)
    if (m < na && (a[m] < 0 || a[m] >= natoms)) ok = false;
  double p[4][3], g[4][3], rho[4][3];
#pragma unroll
  for (int m = 0; m < 4; m++)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      p[m][k] = (ok && m < na) ? x[3 * (size_t)a[m] + k] : 0.0;
      g[m][k] = 0.0;
      rho[m][k] = 0.0;
    }
  double cv = nan;
  if (ok && kd == ANI_MD_RESTRAINT_DISTANCE) {
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = minimg1(p[0][k] - p[1][k], L[k], (pmask >> k) & 1);
    const double l = sqrt(dot3(d, d));
    cv = l;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      g[0][k] = d[k] / l;
      g[1][k] = -g[0][k];
      rho[0][k] = d[k];
    }
  } else if (ok && kd == ANI_MD_RESTRAINT_ANGLE) {
    double u[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      u[k] = minimg1(p[0][k] - p[1][k], L[k], (pmask >> k) & 1);
      w[k] = minimg1(p[2][k] - p[1][k], L[k], (pmask >> k) & 1);
    }
    const double lu = sqrt(dot3(u, u)), lw = sqrt(dot3(w, w));
    double uh[3], wh[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { uh[k] = u[k] / lu; wh[k] = w[k] / lw; }
    const double c = fmin(1.0, fmax(-1.0, dot3(uh, wh)));     // a NaN stays one
    cv = acos(c);
    const double s = sqrt((1.0 - c) * (1.0 + c));
#pragma unroll
    for (int k = 0; k < 3; k++) {
      g[0][k] = (c * uh[k] - wh[k]) / (lu * s);
      g[2][k] = (c * wh[k] - uh[k]) / (lw * s);
      g[1][k] = -(g[0][k] + g[2][k]);
      rho[0][k] = u[k];
      rho[2][k] = w[k];
    }
  } else if (ok) {
    double F[3], G[3], H[3], A[3], B[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      F[k] = minimg1(p[0][k] - p[1][k], L[k], (pmask >> k) & 1);
      G[k] = minimg1(p[1][k] - p[2][k], L[k], (pmask >> k) & 1);
      H[k] = minimg1(p[3][k] - p[2][k], L[k], (pmask >> k) & 1);
    }
    cross3(F, G, A);
    cross3(H, G, B);
    const double lg = sqrt(dot3(G, G)), A2 = dot3(A, A), B2 = dot3(B, B);
    cv = atan2(-(lg * dot3(F, B)), dot3(A, B));
    const double ca = lg / A2, cb = lg / B2, ta = dot3(F, G) / (A2 * lg), tb = dot3(H, G) / (B2 * lg);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double T = ta * A[k] - tb * B[k];
      g[0][k] = -(ca * A[k]);
      g[3][k] = cb * B[k];
      g[1][k] = T - g[0][k];
      g[2][k] = -g[3][k] - T;
      rho[0][k] = F[k];
      rho[2][k] = -G[k];
      rho[3][k] = H[k] - G[k];
    }
  }
  const double kap = kappa[r], dl = restraint_delta(cv, centre[r], kd);
  double chk = dl - dl;
#pragma unroll
  for (int m = 0; m < 4; m++)
#pragma unroll
    for (int k = 0; k < 3; k++) chk += g[m][k] - g[m][k];
  const bool fin = chk == 0.0;
  double fr[4][3], w[9];
#pragma unroll
  for (int m = 0; m < 4; m++)
#pragma unroll
    for (int k = 0; k < 3; k++) fr[m][k] = fin ? -((kap * dl) * g[m][k]) : 0.0;
#pragma unroll
  for (int al = 0; al < 3; al++)
#pragma unroll
    for (int be = 0; be < 3; be++)
      w[3 * al + be] = ((rho[0][al] * fr[0][be] + rho[1][al] * fr[1][be]) + rho[2][al] * fr[2][be]) + rho[3][al] * fr[3][be];
  cv_out[r] = cv;
  e_out[r] = fin ? (0.5 * kap) * (dl * dl) : nan;
#pragma unroll
  for (int m = 0; m < 4; m++)
#pragma unroll
    for (int k = 0; k < 3; k++) fslot[12 * (size_t)r + 3 * m + k] = fr[m][k];
#pragma unroll
  for (int c = 0; c < 9; c++) w_out[9 * (size_t)r + c] = w[c];
}

// blocks [0, gridDim.x - 1): the touched atoms; the last block: the sums, ev, the record and the series row
__global__ __launch_bounds__(256) void restraints_apply_kernel(double* __restrict__ f, int natoms, double* __restrict__ ev, int with_virial,
                                                               const int* __restrict__ touched, const int* __restrict__ row_ptr,
                                                               const int* __restrict__ entries, int ntouched,
                                                               const double* __restrict__ fslot, const double* __restrict__ cv,
                                                               const double* __restrict__ e, const double* __restrict__ w,
                                                               const double* __restrict__ centre, const int* __restrict__ kind, int nr,
                                                               double* __restrict__ rec, double step, double* __restrict__ series_row) {
  if (blockIdx.x + 1 < gridDim.x) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= ntouched) return;
    const int i = touched[t];
    if (i < 0 || i >= natoms) return;       // a word that points outside is skipped here and counted by the last block
    double acc[3] = {0.0, 0.0, 0.0};
    for (int q = row_ptr[t]; q < row_ptr[t + 1]; q++) {
      const int en = entries[q];            // 4 restraint + slot
      if (en < 0 || en >= 4 * nr) continue; // likewise
#pragma unroll
      for (int k = 0; k < 3; k++) acc[k] += fslot[3 * (size_t)en + k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) f[3 * (size_t)i + k] += acc[k];
    return;
  }
  __shared__ double red[4];
  double E = 0.0, W[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bad = 0.0, dmax = 0.0;
  for (int r = threadIdx.x; r < nr; r += 256) {
    const double er = e[r], cr = cv[r];
    E += er;
#pragma unroll
    for (int c = 0; c < 9; c++) W[c] += w[9 * (size_t)r + c];
    if (finite_d(er)) dmax = fmax(dmax, fabs(restraint_delta(cr, centre[r], kind[r])));
    else bad += 1.0;
    if (series_row) { series_row[1 + r] = cr; series_row[1 + nr + r] = er; }
  }
  // the words of the gather table that the threads above skipped: a table that drops force must not pass for a good one
  double skipped = 0.0;
  for (int t = threadIdx.x; t < ntouched; t += 256) {
    const int i = touched[t];
    if (i < 0 || i >= natoms) skipped += 1.0;
  }
  for (int q = row_ptr[0] + threadIdx.x; q < row_ptr[ntouched]; q += 256) {
    const int en = entries[q];
    if (en < 0 || en >= 4 * nr) skipped += 1.0;
  }
  E = block_sum_fixed(E, red);
#pragma unroll
  for (int c = 0; c < 9; c++) W[c] = block_sum_fixed(W[c], red);
  bad = block_sum_fixed(bad, red);
  skipped = block_sum_fixed(skipped, red);
  dmax = block_max(dmax, red);
  if (threadIdx.x != 0) return;
  if (skipped != 0.0) E = __longlong_as_double(0x7ff8000000000000LL);
  ev[0] += E;
  if (with_virial)
#pragma unroll
    for (int c = 0; c < 9; c++) ev[1 + c] += W[c];
  rec[ANI_MD_RESTRAINT_REC_EVALUATIONS] += 1.0;
  rec[ANI_MD_RESTRAINT_REC_EBIAS] = E;
#pragma unroll
  for (int c = 0; c < 9; c++) rec[ANI_MD_RESTRAINT_REC_VIRIAL + c] = W[c];
  rec[ANI_MD_RESTRAINT_REC_NONFINITE] = bad;
  rec[ANI_MD_RESTRAINT_REC_MAX_DELTA] = dmax;
  rec[ANI_MD_RESTRAINT_REC_SKIPPED] = skipped;
  rec[ANI_MD_RESTRAINT_REC_ZERO] = rec[ANI_MD_RESTRAINT_REC_ZERO + 1] = 0.0;
  if (series_row) series_row[0] = step;
}

}  // namespace

extern "C" {

int ani_md_restraints_eval(const double* x, int natoms, const int* atoms, const int* kind, const double* kappa, const double* centre,
                           int nr, const double* len3, const double* box_dev, int periodic_mask, double* cv, double* e, double* fslot,
                           double* w, void* stream) {
  if (nr <= 0) return 0;
  if (!x || !atoms || !kind || !kappa || !centre || !cv || !e || !fslot || !w || (!len3 && !box_dev) || natoms <= 0)
    return (int)hipErrorInvalidValue;
  const double z3[3] = {0.0, 0.0, 0.0};
  const double* l = len3 ? len3 : z3;
  return launch(restraints_eval_kernel, blocks(nr), 256, stream, x, natoms, atoms, kind, kappa, centre, nr, l[0], l[1], l[2], box_dev,
                periodic_mask, cv, e, fslot, w);
}

int ani_md_restraints_apply(double* f, int natoms, double* ev, int with_virial, const int* touched, const int* row_ptr,
                            const int* entries, int ntouched, const double* fslot, const double* cv, const double* e, const double* w,
                            const double* centre, const int* kind, int nr, double* record, double step, double* series_row,
                            void* stream) {
  if (nr <= 0) return 0;
  if (!f || !ev || !touched || !row_ptr || !entries || ntouched <= 0 || !fslot || !cv || !e || !w || !centre || !kind || !record ||
      natoms <= 0)
    return (int)hipErrorInvalidValue;
  return launch(restraints_apply_kernel, dim3((ntouched + 255) / 256 + 1), 256, stream, f, natoms, ev, with_virial, touched, row_ptr,
                entries, ntouched, fslot, cv, e, w, centre, kind, nr, record, step, series_row);
}

}  // extern "C"
