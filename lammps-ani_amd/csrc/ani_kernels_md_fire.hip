// ani_kernels_md_fire.hip — FIRE energy minimisation in the timestep loop (include/ani_md.h, ani_md_fire_*)
#include "ani_md_device.h"

namespace {

// ---- FIRE energy minimisation (include/ani_md.h, ani_md_fire_*) -----------------------------------------------------------
// One iteration is three launches on the caller's stream: reduce (per-block partials of P = sum v.f, vv, ff), velocity (every
// block sums the partials in the same fixed order, takes the same branch, updates v and leaves its max |v| component), move
// (every block takes the maximum over the blocks, limits the step, moves x).  The state record is read by all blocks in the
// velocity launch and written by one thread in the move launch; what the velocity launch decides travels in a decision record
// (work[0 .. FD_N)) that its block 0 writes and the move launch reads: no block reads a scalar that a block of the same launch
// writes, and a stopped record freezes everything (neither launch writes).
enum { FD_STOP = 0, FD_MOVE, FD_ITER, FD_DT, FD_ALPHA, FD_LASTNEG, FD_E, FD_P, FD_VV, FD_FF, FD_NUPHILL, FD_N = 16 };

__global__ void fire_init_kernel(double* __restrict__ state, double dt0, double alpha0) {
  for (int k = 0; k < ANI_MD_FIRE_NSTATE; k++) state[k] = 0.0;
  state[ANI_MD_FIRE_DT] = dt0;
  state[ANI_MD_FIRE_ALPHA] = alpha0;
}

// part[0 .. nblk) = P of the block, [nblk .. 2 nblk) = vv, [2 nblk .. 3 nblk) = ff
__global__ __launch_bounds__(256) void fire_reduce_kernel(const double* __restrict__ v, const double* __restrict__ f, int n,
                                                          const double* __restrict__ state, double* __restrict__ part) {
  if (state[ANI_MD_FIRE_STOP] != 0.0) return;
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x, nblk = gridDim.x;
  double p = 0.0, vv = 0.0, ff = 0.0;
  if (i < n) {
    const double v0 = v[3 * i], v1 = v[3 * i + 1], v2 = v[3 * i + 2], f0 = f[3 * i], f1 = f[3 * i + 1], f2 = f[3 * i + 2];
    p = v0 * f0 + v1 * f1 + v2 * f2;
    vv = v0 * v0 + v1 * v1 + v2 * v2;
    ff = f0 * f0 + f1 * f1 + f2 * f2;
  }
  p = block_sum_fixed(p, red);
  vv = block_sum_fixed(vv, red);
  ff = block_sum_fixed(ff, red);
  if (threadIdx.x == 0) { part[blockIdx.x] = p; part[nblk + blockIdx.x] = vv; part[2 * nblk + blockIdx.x] = ff; }
}

__global__ __launch_bounds__(256) void fire_velocity_kernel(double* __restrict__ x, double* __restrict__ v, const double* __restrict__ f,
                                                            const double* __restrict__ fm, int n, const double* __restrict__ ev,
                                                            ani_md_fire_params p, const double* __restrict__ state,
                                                            const double* __restrict__ part, double* __restrict__ dec,
                                                            double* __restrict__ vmaxp) {
  if (state[ANI_MD_FIRE_STOP] != 0.0) return;   // frozen: the decision record keeps saying "no move"
  __shared__ double red[4];
  const int nblk = gridDim.x;
  double P = 0.0, vv = 0.0, ff = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) { P += part[b]; vv += part[nblk + b]; ff += part[2 * nblk + b]; }
  P = block_sum_fixed(P, red);
  vv = block_sum_fixed(vv, red);
  ff = block_sum_fixed(ff, red);
  const double E = ev[0], e_prev = state[ANI_MD_FIRE_E_PREV], done = state[ANI_MD_FIRE_ITERATIONS], k = done + 1.0;
  double dt = state[ANI_MD_FIRE_DT], alpha = state[ANI_MD_FIRE_ALPHA], last_neg = state[ANI_MD_FIRE_LAST_NEGATIVE];
  double nuphill = state[ANI_MD_FIRE_UPHILL];
  const double dtv_prev = state[ANI_MD_FIRE_DTV];
  int stop = 0;
  if (!finite_d(E) || !finite_d(ff)) stop = 4;
  else if (ff < p.ftol * p.ftol) stop = 2;
  else if (k > 1.0 && (k - 1.0 - last_neg) > (double)p.delaystep && fabs(E - e_prev) < p.etol * 0.5 * (fabs(E) + fabs(e_prev) + 1e-8)) stop = 1;
  else if (done == (double)p.maxiter) stop = 3;
  const bool downhill = P > 0.0;
  double s1 = 1.0, s2 = 0.0;
  if (!stop) {
    if (downhill) {
      s1 = 1.0 - alpha;
      s2 = ff <= 1e-20 ? 0.0 : alpha * sqrt(vv / ff);
      if (k - last_neg > (double)p.delaystep) { dt = fmin(dt * p.dtgrow, p.dtmax); alpha *= p.alphashrink; }
    } else {
      nuphill += 1.0;
      last_neg = k;
      if (!(p.initialdelay && k <= (double)p.delaystep)) {
        alpha = p.alpha0;
        if (dt * p.dtshrink >= p.dtmin) dt *= p.dtshrink;
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    dec[FD_STOP] = (double)stop; dec[FD_MOVE] = stop ? 0.0 : 1.0; dec[FD_ITER] = stop ? done : k; dec[FD_DT] = dt; dec[FD_ALPHA] = alpha;
    dec[FD_LASTNEG] = last_neg; dec[FD_E] = E; dec[FD_P] = P; dec[FD_VV] = vv; dec[FD_FF] = ff; dec[FD_NUPHILL] = nuphill;
  }
  if (stop) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  double vm = 0.0;
  if (i < n) {
    const double a = dt * fm[i];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double fc = f[3 * i + c];
      double vc = v[3 * i + c];
      if (!downhill) {
        if (p.halfstepback) x[3 * i + c] -= 0.5 * dtv_prev * vc;
        vc = 0.0;
      }
      vc += a * fc;
      if (downhill) vc = s1 * vc + s2 * fc;
      v[3 * i + c] = vc;
      vm = fmax(vm, fabs(vc));
    }
  }
  vm = block_max(vm, red);
  if (threadIdx.x == 0) vmaxp[blockIdx.x] = vm;
}

__global__ __launch_bounds__(256) void fire_move_kernel(double* __restrict__ x, const double* __restrict__ v, int n, double dmax,
                                                        const double* __restrict__ dec, const double* __restrict__ vmaxp,
                                                        double* __restrict__ state, const double* __restrict__ xb,
                                                        double* __restrict__ d2max) {
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (dec[FD_MOVE] == 0.0) {
    // the iteration that stops commits its reason and the sums and energy it stopped on, once; nothing after that
    if (writer && state[ANI_MD_FIRE_STOP] == 0.0 && dec[FD_STOP] != 0.0) {
      state[ANI_MD_FIRE_E_CUR] = dec[FD_E]; state[ANI_MD_FIRE_P] = dec[FD_P];
      state[ANI_MD_FIRE_VV] = dec[FD_VV]; state[ANI_MD_FIRE_FF] = dec[FD_FF];
      if (dec[FD_ITER] == 0.0) { state[ANI_MD_FIRE_E_FIRST] = dec[FD_E]; state[ANI_MD_FIRE_FF_FIRST] = dec[FD_FF]; }
      state[ANI_MD_FIRE_STOP] = dec[FD_STOP];
    }
    return;
  }
  __shared__ double red[4];
  const int nblk = gridDim.x;
  double vmax = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) vmax = fmax(vmax, vmaxp[b]);
  vmax = block_max(vmax, red);
  double dtv = dec[FD_DT];
  const bool limited = dtv * vmax > dmax;
  if (limited) dtv = dmax / vmax;
  const int i = blockIdx.x * 256 + threadIdx.x;
  double d2 = 0.0;
  if (i < n) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double xc = x[3 * i + c] + dtv * v[3 * i + c];
      x[3 * i + c] = xc;
      const double d = xb ? xc - xb[3 * i + c] : 0.0;
      d2 += d * d;
    }
  }
  if (writer) {
    state[ANI_MD_FIRE_ITERATIONS] = dec[FD_ITER]; state[ANI_MD_FIRE_DT] = dec[FD_DT]; state[ANI_MD_FIRE_ALPHA] = dec[FD_ALPHA];
    state[ANI_MD_FIRE_LAST_NEGATIVE] = dec[FD_LASTNEG]; state[ANI_MD_FIRE_E_PREV] = dec[FD_E]; state[ANI_MD_FIRE_E_CUR] = dec[FD_E];
    state[ANI_MD_FIRE_P] = dec[FD_P]; state[ANI_MD_FIRE_VV] = dec[FD_VV]; state[ANI_MD_FIRE_FF] = dec[FD_FF];
    state[ANI_MD_FIRE_DTV] = dtv; state[ANI_MD_FIRE_UPHILL] = dec[FD_NUPHILL]; state[ANI_MD_FIRE_VMAX] = vmax;
    if (limited) state[ANI_MD_FIRE_LIMITED] += 1.0;
    if (dec[FD_ITER] == 1.0) { state[ANI_MD_FIRE_E_FIRST] = dec[FD_E]; state[ANI_MD_FIRE_FF_FIRST] = dec[FD_FF]; }
  }
  if (!d2max) return;
  d2 = block_max(d2, red);
  if (threadIdx.x == 0) raise_d2max(d2, d2max);
}

// ani_md_check with the FIRE state record behind it: one pinned read of the host brings both
__global__ void fire_check_kernel(double* __restrict__ d2max, const double* __restrict__ ev, const double* __restrict__ state,
                                  double* __restrict__ out) {
  const double e = ev[0];
  out[0] = finite_d(e) ? d2max[0] : __longlong_as_double(0x7ff0000000000000LL);
  d2max[0] = 0.0;
  for (int k = 0; k < ANI_MD_FIRE_NSTATE; k++) out[1 + k] = state[k];
}

}  // namespace

extern "C" {

int ani_md_fire_work_size(int nlocal) { return FD_N + 4 * nblocks(nlocal); }

int ani_md_fire_init(double* state, double* v, int nlocal, const ani_md_fire_params* p, void* stream) {
  if (!state || !p) return (int)hipErrorInvalidValue;
  if (nlocal > 0 && v) {
    const hipError_t rc = hipMemsetAsync(v, 0, sizeof(double) * 3 * (size_t)nlocal, (hipStream_t)stream);
    if (rc != hipSuccess) return (int)rc;
  }
  return launch(fire_init_kernel, dim3(1), 1, stream, state, p->dt0, p->alpha0);
}

int ani_md_fire_iterate(double* x, double* v, const double* f, const double* fm, int nlocal, const double* ev,
                        const ani_md_fire_params* p, double* state, double* work, const double* x_built, double* d2max,
                        void* stream) {
  if (nlocal <= 0) return 0;
  if (!p || !state || !work) return (int)hipErrorInvalidValue;
  const int nblk = nblocks(nlocal);
  double* dec = work;
  double* part = work + FD_N;
  double* vmaxp = part + 3 * nblk;
  enqueue(fire_reduce_kernel, dim3(nblk), 256, stream, v, f, nlocal, state, part);
  enqueue(fire_velocity_kernel, dim3(nblk), 256, stream, x, v, f, fm, nlocal, ev, *p, state, part, dec, vmaxp);
  return launch(fire_move_kernel, dim3(nblk), 256, stream, x, v, nlocal, p->dmax, dec, vmaxp, state, x_built, d2max);
}

int ani_md_fire_check(double* d2max, const double* ev, const double* state, double* out, void* stream) {
  return launch(fire_check_kernel, dim3(1), 1, stream, d2max, ev, state, out);
}

}  // extern "C"
