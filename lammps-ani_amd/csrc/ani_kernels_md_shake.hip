// ani_kernels_md_shake.hip — bond constraints of the timestep loop in the RATTLE form (include/ani_md.h, ani_md_shake_positions /
// ani_md_rattle_velocities)
#include "ani_md_device.h"

namespace {

// ---- bond constraints in the RATTLE form (include/ani_md.h, ani_md_shake_positions / ani_md_rattle_velocities) --------------
// One thread per cluster (a centre and K <= 3 partners), everything in registers: the K unknowns of a cluster couple only through
// its centre, so the K x K system is solved directly.  Slots that a cluster does not use are carried as rows and columns of the
// identity with a zero right-hand side: one 3 x 3 solve serves K = 1, 2 and 3, and the unused unknowns stay exactly zero.
static_assert(ANI_MD_SHAKE_NSTATS == 4, "stats layout of include/ani_md.h");

// y = A^-1 b by the adjugate (the systems here are diagonally dominant: the partners are the light atoms)
__device__ __forceinline__ void solve3(const double (&A)[3][3], const double (&b)[3], double (&y)[3]) {
  const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2],
               c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
  const double inv = 1.0 / (A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02);
  y[0] = (c00 * b[0] + (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * b[1] + (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * b[2]) * inv;
  y[1] = (c01 * b[0] + (A[0][0] * A[2][2] - A[0][2] * A[2][0]) * b[1] + (A[0][2] * A[1][0] - A[0][0] * A[1][2]) * b[2]) * inv;
  y[2] = (c02 * b[0] + (A[0][1] * A[2][0] - A[0][0] * A[2][1]) * b[1] + (A[0][0] * A[1][1] - A[0][1] * A[1][0]) * b[2]) * inv;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long a) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)(a & 0xffffffffULL), off), hi = __shfl_xor((unsigned)(a >> 32), off);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    a = o > a ? o : a;
  }
  return a;
}

__global__ __launch_bounds__(256) void shake_positions_kernel(double* __restrict__ x, double* __restrict__ v, const int* __restrict__ cl,
                                                              const double* __restrict__ dl, int nc, const double* __restrict__ w,
                                                              double dt, double tol, int maxiter, double L0, double L1, double L2,
                                                              int pmask, const double* __restrict__ xb, double* __restrict__ d2max,
                                                              unsigned long long* __restrict__ stats) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  double d2 = 0.0;
  unsigned long long resbits = 0ULL;
  unsigned iters = 0, unconverged = 0;
  if (c < nc) {
    const double L[3] = {L0, L1, L2};
    const int4 a4 = reinterpret_cast<const int4*>(cl)[c];
    const int ac = a4.x, ap[3] = {a4.y, a4.z, a4.w};
    const double wc = w[ac];
    double xc[3], s[3][3], rp[3][3], xp[3][3], wp[3], dd[3];
#pragma unroll
    for (int m = 0; m < 3; m++) xc[m] = x[3 * (size_t)ac + m];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      wp[k] = 0.0; dd[k] = 0.0;
#pragma unroll
      for (int m = 0; m < 3; m++) { s[k][m] = 0.0; rp[k][m] = 0.0; xp[k][m] = 0.0; }
      if (ap[k] < 0) continue;
      wp[k] = w[ap[k]];
      const double dk = dl[3 * (size_t)c + k];
      dd[k] = dk * dk;
#pragma unroll
      for (int m = 0; m < 3; m++) {
        const int per = (pmask >> m) & 1;
        xp[k][m] = x[3 * (size_t)ap[k] + m];
        const double now = xc[m] - xp[k][m];
        // x0 = x' - dt v of both ends: the bond of the step's start
        const double old = v ? (xc[m] - dt * v[3 * (size_t)ac + m]) - (xp[k][m] - dt * v[3 * (size_t)ap[k] + m]) : now;
        rp[k][m] = minimg1(now, L[m], per);
        s[k][m] = minimg1(old, L[m], per);
      }
    }
    double g[3] = {0.0, 0.0, 0.0};
    for (;;) {
      double sum[3], r[3][3], F[3];
#pragma unroll
      for (int m = 0; m < 3; m++) sum[m] = wc * (g[0] * s[0][m] + g[1] * s[1][m] + g[2] * s[2][m]);
      bool ok = true;
      unsigned long long cur = 0ULL;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        double rr = 0.0;
#pragma unroll
        for (int m = 0; m < 3; m++) {
          r[k][m] = rp[k][m] + sum[m] + wp[k] * g[k] * s[k][m];
          rr += r[k][m] * r[k][m];
        }
        F[k] = rr - dd[k];
        if (ap[k] >= 0) {
          ok = ok && fabs(F[k]) <= tol * dd[k];     // false for a NaN: such a cluster runs to maxiter and is counted
          const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(F[k] / dd[k]));
          cur = bits > cur ? bits : cur;            // non-negative doubles order like their bit patterns, a NaN above them all
        }
      }
      resbits = cur;
      if (ok) break;
      if ((int)iters >= maxiter) { unconverged = 1; break; }
      double J[3][3], mF[3], dg[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        mF[k] = -F[k];
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const double wj = j == k ? wc + wp[k] : wc;
          J[k][j] = 2.0 * wj * (r[k][0] * s[j][0] + r[k][1] * s[j][1] + r[k][2] * s[j][2]);
        }
        if (ap[k] < 0) { J[k][k] = 1.0; mF[k] = 0.0; }
      }
      solve3(J, mF, dg);
#pragma unroll
      for (int k = 0; k < 3; k++) g[k] += dg[k];
      iters++;
    }
    const double rdt = 1.0 / dt;
    double dxc[3];
#pragma unroll
    for (int m = 0; m < 3; m++) dxc[m] = wc * (g[0] * s[0][m] + g[1] * s[1][m] + g[2] * s[2][m]);
    double dc2 = 0.0;
#pragma unroll
    for (int m = 0; m < 3; m++) {
      const double xn = xc[m] + dxc[m];
      x[3 * (size_t)ac + m] = xn;
      if (v) v[3 * (size_t)ac + m] += dxc[m] * rdt;
      const double e = xb ? xn - xb[3 * (size_t)ac + m] : 0.0;
      dc2 += e * e;
    }
    d2 = dc2;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (ap[k] < 0) continue;
      double dp2 = 0.0;
#pragma unroll
      for (int m = 0; m < 3; m++) {
        const double dxp = -(wp[k] * g[k] * s[k][m]);
        const double xn = xp[k][m] + dxp;
        x[3 * (size_t)ap[k] + m] = xn;
        if (v) v[3 * (size_t)ap[k] + m] += dxp * rdt;
        const double e = xb ? xn - xb[3 * (size_t)ap[k] + m] : 0.0;
        dp2 += e * e;
      }
      d2 = fmax(d2, dp2);
    }
  }
  // workgroup reductions of d2 and the statistics together, then at most one integer atomic per word and workgroup (none once
  // the running value is larger)
  for (int off = 32; off > 0; off >>= 1) {
    d2 = fmax(d2, __shfl_xor(d2, off));
    const unsigned it = __shfl_xor(iters, off);
    iters = it > iters ? it : iters;
    unconverged += __shfl_xor(unconverged, off);
  }
  resbits = wave_max_u64(resbits);
  __shared__ double wmax[4];
  __shared__ unsigned long long wres[4];
  __shared__ unsigned wit[4], wun[4];
  if ((threadIdx.x & 63) == 0) {
    const int wv = threadIdx.x >> 6;
    wmax[wv] = d2; wres[wv] = resbits; wit[wv] = iters; wun[wv] = unconverged;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (d2max && xb) raise_d2max(fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3])), d2max);
  if (!stats) return;
  unsigned long long res = wres[0];
  unsigned it = wit[0];
  for (int k = 1; k < 4; k++) { res = wres[k] > res ? wres[k] : res; it = wit[k] > it ? wit[k] : it; }
  const unsigned un = wun[0] + wun[1] + wun[2] + wun[3];
  volatile unsigned long long* seen = stats;
  if (un) atomicAdd(&stats[0], (unsigned long long)un);
  if ((unsigned long long)it > seen[1]) atomicMax(&stats[1], (unsigned long long)it);
  if (res > seen[2]) atomicMax(&stats[2], res);
  if (blockIdx.x == 0) atomicAdd(&stats[3], 1ULL);
}

__global__ __launch_bounds__(256) void rattle_velocities_kernel(const double* __restrict__ x, double* __restrict__ v,
                                                                const int* __restrict__ cl, int nc, const double* __restrict__ w,
                                                                double L0, double L1, double L2, int pmask) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nc) return;
  const double L[3] = {L0, L1, L2};
  const int4 a4 = reinterpret_cast<const int4*>(cl)[c];
  const int ac = a4.x, ap[3] = {a4.y, a4.z, a4.w};
  const double wc = w[ac];
  double xc[3], vc[3], r[3][3], vp[3][3], wp[3], b[3];
#pragma unroll
  for (int m = 0; m < 3; m++) { xc[m] = x[3 * (size_t)ac + m]; vc[m] = v[3 * (size_t)ac + m]; }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    wp[k] = 0.0; b[k] = 0.0;
#pragma unroll
    for (int m = 0; m < 3; m++) { r[k][m] = 0.0; vp[k][m] = 0.0; }
    if (ap[k] < 0) continue;
    wp[k] = w[ap[k]];
#pragma unroll
    for (int m = 0; m < 3; m++) {
      r[k][m] = minimg1(xc[m] - x[3 * (size_t)ap[k] + m], L[m], (pmask >> m) & 1);
      vp[k][m] = v[3 * (size_t)ap[k] + m];
      b[k] -= r[k][m] * (vc[m] - vp[k][m]);
    }
  }
  double A[3][3], h[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double wj = j == k ? wc + wp[k] : wc;
      A[k][j] = wj * (r[k][0] * r[j][0] + r[k][1] * r[j][1] + r[k][2] * r[j][2]);
    }
    if (ap[k] < 0) A[k][k] = 1.0;
  }
  solve3(A, b, h);
#pragma unroll
  for (int m = 0; m < 3; m++) v[3 * (size_t)ac + m] = vc[m] + wc * (h[0] * r[0][m] + h[1] * r[1][m] + h[2] * r[2][m]);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (ap[k] < 0) continue;
#pragma unroll
    for (int m = 0; m < 3; m++) v[3 * (size_t)ap[k] + m] = vp[k][m] - wp[k] * h[k] * r[k][m];
  }
}

}  // namespace

extern "C" {

int ani_md_shake_positions(double* x, double* v, const int* cl, const double* d, int nc, const double* w, double dt, double tol,
                           int maxiter, const double* len3, int periodic_mask, const double* x_built, double* d2max,
                           unsigned long long* stats, void* stream) {
  if (nc <= 0) return 0;
  if (!x || !cl || !d || !w || !len3 || !(dt > 0.0)) return (int)hipErrorInvalidValue;
  return launch(shake_positions_kernel, blocks(nc), 256, stream, x, v, cl, d, nc, w, dt, tol, maxiter, len3[0], len3[1], len3[2],
                periodic_mask, x_built, d2max, stats);
}

int ani_md_rattle_velocities(const double* x, double* v, const int* cl, const double* d, int nc, const double* w,
                             const double* len3, int periodic_mask, void* stream) {
  (void)d;
  if (nc <= 0) return 0;
  if (!x || !v || !cl || !w || !len3) return (int)hipErrorInvalidValue;
  return launch(rattle_velocities_kernel, blocks(nc), 256, stream, x, v, cl, nc, w, len3[0], len3[1], len3[2], periodic_mask);
}

}  // extern "C"
