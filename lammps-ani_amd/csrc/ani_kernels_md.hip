// ani_kernels_md.hip — the timestep loop's own kernels (include/ani_md.h): what LAMMPS' fix nve, fix langevin,
// Neighbor::check_distance and Comm do around PairANI::compute in the reference's runs
// (examples/benchmark/in.lammps:24-27,54-72).  Test / bench infrastructure of the LAMMPS-free loop, not the pair style.
#include <hip/hip_runtime.h>

#include "../../include/ani_md.h"

namespace {

// ---- shared pieces ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite_d(double a) { return a - a == 0.0; }

// sum over the 256 threads of a block, the same order every time: xor butterflies inside a wave, then the four waves in order
__device__ __forceinline__ double block_sum_fixed(double a, double* red) {
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
  __syncthreads();   // red may still be read from the call before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double block_max(double a, double* red) {
  for (int off = 32; off > 0; off >>= 1) a = fmax(a, __shfl_xor(a, off));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// The displacement fold.  One thread of a workgroup hands in the workgroup's maximum: at most one atomic per workgroup -- and none
// once the running maximum is larger (it only grows between two looks of the host: a stale read costs an atomic, never a missed
// one).  1 563 same-address atomics made initial_integrate_kernel 21 us at 100 002 atoms.  Non-negative doubles order like their
// bit patterns.
__device__ __forceinline__ void raise_d2max(double d2, double* __restrict__ d2max) {
  if (d2 > *reinterpret_cast<volatile double*>(d2max))
    atomicMax(reinterpret_cast<unsigned long long*>(d2max), (unsigned long long)__double_as_longlong(d2));
}
// every thread's d2: workgroup maximum (one barrier), then raise_d2max by thread 0
__device__ __forceinline__ void fold_d2max(double d2, double* __restrict__ d2max) {
  for (int off = 32; off > 0; off >>= 1) d2 = fmax(d2, __shfl_xor(d2, off));
  __shared__ double wmax[4];
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = d2;
  __syncthreads();
  if (threadIdx.x == 0) raise_d2max(fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3])), d2max);
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {   // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
// fix langevin's random numbers: a key per (seed, step, atom), a uniform draw in [-0.5, 0.5) per component of it
__device__ __forceinline__ unsigned long long langevin_key(unsigned long long seed, unsigned long long step, long long atom) {
  return mix64(seed + 0x9E3779B97F4A7C15ULL * (step + 1)) ^ (0xD1B54A32D192ED03ULL * (unsigned long long)atom);
}
__device__ __forceinline__ double langevin_draw(unsigned long long key, int k) {
  const unsigned long long h = mix64(key + 0x9E3779B97F4A7C15ULL * (k + 1));
  return (double)(h >> 11) * (1.0 / 9007199254740992.0) - 0.5;
}

// element t of an [n][3] block of doubles, as an offset into the array that the row index idx points into: 3 idx[t / 3] + t % 3
__device__ __forceinline__ long long through3(const long long* __restrict__ idx, int t) {
  const int g = t / 3, k = t - 3 * g;
  return 3 * idx[g] + k;
}

__global__ __launch_bounds__(256) void initial_integrate_kernel(double* __restrict__ x, double* __restrict__ v,
                                                                const double* __restrict__ f, const double* __restrict__ dtfm,
                                                                double dt, int n, const double* __restrict__ xb,
                                                                double* __restrict__ d2max) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double d2 = 0.0;
  if (i < n) {
    const double s = dtfm[i];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double vk = v[3 * i + k] + s * f[3 * i + k];
      const double xk = x[3 * i + k] + dt * vk;
      v[3 * i + k] = vk;
      x[3 * i + k] = xk;
      const double d = xk - xb[3 * i + k];
      d2 += d * d;
    }
  }
  fold_d2max(d2, d2max);
}

__global__ __launch_bounds__(256) void final_integrate_kernel(double* __restrict__ v, double* __restrict__ f,
                                                              const double* __restrict__ dtfm, int n, int langevin,
                                                              const double* __restrict__ g1, const double* __restrict__ g2,
                                                              const long long* __restrict__ tag, unsigned long long seed,
                                                              unsigned long long step) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double s = dtfm[i];
  const unsigned long long key = langevin_key(seed, step, tag ? tag[i] : i);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double fk = f[3 * i + k];
    const double vk = v[3 * i + k];
    if (langevin) {
      const double r = langevin_draw(key, k);
      fk += g1[i] * vk + g2[i] * r;
      f[3 * i + k] = fk;
    }
    v[3 * i + k] = vk + s * fk;
  }
}

// final_integrate of step n and initial_integrate of step n + 1 in one pass over the owned atoms (nothing happens between
// them in a run without per-step output): f += thermostat;  v += s f  (the full-step velocity, not stored);  v += s f;  x += dt v
__global__ __launch_bounds__(256) void final_initial_integrate_kernel(double* __restrict__ x, double* __restrict__ v, double* __restrict__ f,
                                                                      const double* __restrict__ dtfm, double dt, int n, int langevin,
                                                                      const double* __restrict__ g1, const double* __restrict__ g2,
                                                                      const long long* __restrict__ tag, unsigned long long seed,
                                                                      unsigned long long step, const double* __restrict__ xb,
                                                                      double* __restrict__ d2max) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double d2 = 0.0;
  if (i < n) {
    const double s = dtfm[i];
    const unsigned long long key = langevin_key(seed, step, tag ? tag[i] : i);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      double fk = f[3 * i + k];
      double vk = v[3 * i + k];
      if (langevin) {
        const double r = langevin_draw(key, k);
        fk += g1[i] * vk + g2[i] * r;
        f[3 * i + k] = fk;
      }
      vk += s * fk;            // final_integrate of the step that ends
      vk += s * fk;            // initial_integrate of the step that begins (same rounding as the two kernels)
      const double xk = x[3 * i + k] + dt * vk;
      v[3 * i + k] = vk;
      x[3 * i + k] = xk;
      const double d = xk - xb[3 * i + k];
      d2 += d * d;
    }
  }
  fold_d2max(d2, d2max);
}

__global__ __launch_bounds__(256) void forward_ghosts_kernel(double* __restrict__ x, const long long* __restrict__ owner,
                                                             const double* __restrict__ shift, int nlocal, int nghost) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * nghost) return;
  x[3 * (size_t)nlocal + t] = x[through3(owner, t)] + shift[t];
}

__global__ __launch_bounds__(256) void pack_ghosts_kernel(const double* __restrict__ x, const long long* __restrict__ owner,
                                                          const double* __restrict__ shift, int nsend, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * nsend) return;
  out[t] = x[through3(owner, t)] + shift[t];
}

__global__ __launch_bounds__(256) void unpack_reverse_kernel(double* __restrict__ f, const long long* __restrict__ owner, int nsend,
                                                             const double* __restrict__ in) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * nsend) return;
  atomicAdd(&f[through3(owner, t)], in[t]);   // an atom can be a ghost of several bricks / images
}

__global__ __launch_bounds__(256) void reverse_ghosts_kernel(double* __restrict__ f, const long long* __restrict__ owner,
                                                             int nlocal, int nghost) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * nghost) return;
  atomicAdd(&f[through3(owner, t)], f[3 * (size_t)nlocal + t]);
}

// the same with the ghost block in the caller's order: message slot g is ghost ghost_of[g] (two indices through one g: spelt out)
__global__ __launch_bounds__(256) void reverse_ghosts_ordered_kernel(double* __restrict__ f, const long long* __restrict__ owner,
                                                                     const long long* __restrict__ ghost_of, int nlocal, int nghost) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * nghost) return;
  const int g = t / 3, k = t - 3 * g;
  atomicAdd(&f[3 * owner[g] + k], f[3 * ((size_t)nlocal + (size_t)ghost_of[g]) + k]);
}

// rows[k] = src[idx[k]] (gather) / dst[idx[k]] = rows[k] (scatter): three doubles per row
__global__ __launch_bounds__(256) void gather_rows_kernel(const double* __restrict__ src, const long long* __restrict__ idx, int n,
                                                          double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * n) return;
  out[t] = src[through3(idx, t)];
}
__global__ __launch_bounds__(256) void scatter_rows_kernel(double* __restrict__ dst, const long long* __restrict__ idx, int n,
                                                           const double* __restrict__ in) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * n) return;
  const long long o = through3(idx, t);
  dst[o] = in[t];
}


// ---- re-neighbouring of the stand-in loop, natively (LAMMPS: Domain::pbc, Comm::borders) ---------------------------------
__global__ __launch_bounds__(256) void wrap_kernel(double* __restrict__ x, int n, double lo0, double lo1, double lo2, double l0, double l1,
                                                   double l2, int pmask) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * n) return;
  const int k = t % 3;
  if (!((pmask >> k) & 1)) return;
  const double lo = k == 0 ? lo0 : (k == 1 ? lo1 : lo2), L = k == 0 ? l0 : (k == 1 ? l1 : l2);
  double v = x[t];
  v -= floor((v - lo) / L) * L;
  if (v >= lo + L) v = lo;   // a coordinate that rounds up onto the upper face
  if (v < lo) v = lo;        // a quotient that rounds up to the integer: the image a hair under the upper face comes out a hair under lo
  x[t] = v;
}

// Ghost shell: atom a is a ghost of combination c (a brick of the decomposition and an image shift) when its UNSHIFTED position
// lies in [clo[c], chi[c]) in every dimension.  Hits are listed combination-major, atoms ascending (the order the exchange and
// the receiver's ghost block agree on): count per (combination, block of 256 atoms), scan, fill.
__device__ __forceinline__ bool shell_hit(const double* __restrict__ x, int a, int n, const double* __restrict__ clo,
                                          const double* __restrict__ chi, int c) {
  if (a >= n) return false;
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double v = x[3 * a + k];
    in = in && v >= clo[3 * c + k] && v < chi[3 * c + k];
  }
  return in;
}
__global__ __launch_bounds__(256) void shell_count_kernel(const double* __restrict__ x, int n, const double* __restrict__ clo,
                                                          const double* __restrict__ chi, int nblk, int* __restrict__ blk_cnt) {
  const int b = blockIdx.x, c = blockIdx.y;
  const bool hit = shell_hit(x, b * 256 + threadIdx.x, n, clo, chi, c);
  __shared__ int wc[4];
  const int cnt = __popcll(__ballot(hit));
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[c * nblk + b] = wc[0] + wc[1] + wc[2] + wc[3];
}
// exclusive scan of blk_cnt[ncombo * nblk] by one block; out_counts[0] = total, out_counts[1 + c] = hits of combination c
__global__ __launch_bounds__(1024) void shell_scan_kernel(const int* __restrict__ blk_cnt, int* __restrict__ blk_off, int ncombo, int nblk,
                                                          int* __restrict__ out_counts) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const int total_n = ncombo * nblk;
  for (int base = 0; base < total_n; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < total_n ? blk_cnt[i] : 0;
    // inclusive scan inside the wave, then over the waves
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off);
      if ((threadIdx.x & 63) >= off) incl += t;
    }
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    int before = carry_s, tot = 0;
    for (int w = 0; w < 16; w++) { if (w < (int)(threadIdx.x >> 6)) before += wsum[w]; tot += wsum[w]; }
    if (i < total_n) blk_off[i] = before + incl - v;
    __syncthreads();
    if (threadIdx.x == 0) carry_s += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) out_counts[0] = carry_s;
  __syncthreads();
  for (int c = threadIdx.x; c < ncombo; c += 1024) {
    const int beg = blk_off[c * nblk];
    const int end = c + 1 < ncombo ? blk_off[(c + 1) * nblk] : carry_s;
    out_counts[1 + c] = end - beg;
  }
}
__global__ __launch_bounds__(256) void shell_fill_kernel(const double* __restrict__ x, int n, const double* __restrict__ clo,
                                                         const double* __restrict__ chi, const double* __restrict__ cshift, int nblk,
                                                         const int* __restrict__ blk_off, long long* __restrict__ send_idx,
                                                         double* __restrict__ send_shift) {
  const int b = blockIdx.x, c = blockIdx.y, a = b * 256 + threadIdx.x;
  const bool hit = shell_hit(x, a, n, clo, chi, c);
  __shared__ int wc[4];
  const unsigned long long m = __ballot(hit);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wc[wave] = __popcll(m);
  __syncthreads();
  if (!hit) return;
  int pos = blk_off[c * nblk + b] + __popcll(m & ((1ULL << lane) - 1ULL));
  for (int w = 0; w < wave; w++) pos += wc[w];
  send_idx[pos] = a;
  send_shift[3 * pos] = cshift[3 * c]; send_shift[3 * pos + 1] = cshift[3 * c + 1]; send_shift[3 * pos + 2] = cshift[3 * c + 2];
}
// one rank: the ghosts are images of owned atoms -- positions and species appended behind the owned block
__global__ __launch_bounds__(256) void append_ghosts_kernel(double* __restrict__ x, int* __restrict__ species, int nlocal,
                                                            const long long* __restrict__ owner, const double* __restrict__ shift, int nghost) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nghost) return;
  const long long o = owner[g];
#pragma unroll
  for (int k = 0; k < 3; k++) x[3 * (size_t)(nlocal + g) + k] = x[3 * o + k] + shift[3 * g + k];
  species[nlocal + g] = species[o];
}
// Neighbor::decide's look at the loop: *out = the running displacement maximum (then zeroed), or +inf when the last energy is not
// finite (a capacity overflow or a blown-up step: the device entry points cannot return an error).  fire_check_kernel has the same
// three lines with finite_d for the test: the compiler does not fold `e == e` away, so one body would change one of the two.
__global__ void check_kernel(double* __restrict__ d2max, const double* __restrict__ ev, double* __restrict__ out) {
  const double e = ev[0];
  const bool finite = e == e && e - e == 0.0;
  out[0] = finite ? d2max[0] : __longlong_as_double(0x7ff0000000000000LL);
  d2max[0] = 0.0;
}

// ---- FIRE energy minimisation (include/ani_md.h, ani_md_fire_*) -----------------------------------------------------------
// One iteration is three launches on the caller's stream: reduce (per-block partials of P = sum v.f, vv, ff), velocity (every
// block sums the partials in the same fixed order, takes the same branch, updates v and leaves its max |v| component), move
// (every block takes the maximum over the blocks, limits the step, moves x).  The state record is read by all blocks in the
// velocity launch and written by one thread in the move launch; what the velocity launch decides travels in a decision record
// (work[0 .. FD_N)) that its block 0 writes and the move launch reads: no block reads a scalar that a block of the same launch
// writes, and a stopped record freezes everything (neither launch writes).
enum { FS_ITER = 0, FS_DT, FS_ALPHA, FS_LASTNEG, FS_EPREV, FS_ECUR, FS_P, FS_VV, FS_FF, FS_DTV, FS_NUPHILL, FS_NLIMITED, FS_STOP,
       FS_EFIRST, FS_FFFIRST, FS_VMAX, FS_N };
static_assert(FS_N == ANI_MD_FIRE_NSTATE, "state layout of include/ani_md.h");
enum { FD_STOP = 0, FD_MOVE, FD_ITER, FD_DT, FD_ALPHA, FD_LASTNEG, FD_E, FD_P, FD_VV, FD_FF, FD_NUPHILL, FD_N = 16 };

__global__ void fire_init_kernel(double* __restrict__ state, double dt0, double alpha0) {
  for (int k = 0; k < FS_N; k++) state[k] = 0.0;
  state[FS_DT] = dt0;
  state[FS_ALPHA] = alpha0;
}

// part[0 .. nblk) = P of the block, [nblk .. 2 nblk) = vv, [2 nblk .. 3 nblk) = ff
__global__ __launch_bounds__(256) void fire_reduce_kernel(const double* __restrict__ v, const double* __restrict__ f, int n,
                                                          const double* __restrict__ state, double* __restrict__ part) {
  if (state[FS_STOP] != 0.0) return;
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
  if (state[FS_STOP] != 0.0) return;   // frozen: the decision record keeps saying "no move"
  __shared__ double red[4];
  const int nblk = gridDim.x;
  double P = 0.0, vv = 0.0, ff = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) { P += part[b]; vv += part[nblk + b]; ff += part[2 * nblk + b]; }
  P = block_sum_fixed(P, red);
  vv = block_sum_fixed(vv, red);
  ff = block_sum_fixed(ff, red);
  const double E = ev[0], e_prev = state[FS_EPREV], done = state[FS_ITER], k = done + 1.0;
  double dt = state[FS_DT], alpha = state[FS_ALPHA], last_neg = state[FS_LASTNEG], nuphill = state[FS_NUPHILL];
  const double dtv_prev = state[FS_DTV];
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
    if (writer && state[FS_STOP] == 0.0 && dec[FD_STOP] != 0.0) {
      state[FS_ECUR] = dec[FD_E]; state[FS_P] = dec[FD_P]; state[FS_VV] = dec[FD_VV]; state[FS_FF] = dec[FD_FF];
      if (dec[FD_ITER] == 0.0) { state[FS_EFIRST] = dec[FD_E]; state[FS_FFFIRST] = dec[FD_FF]; }
      state[FS_STOP] = dec[FD_STOP];
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
    state[FS_ITER] = dec[FD_ITER]; state[FS_DT] = dec[FD_DT]; state[FS_ALPHA] = dec[FD_ALPHA]; state[FS_LASTNEG] = dec[FD_LASTNEG];
    state[FS_EPREV] = dec[FD_E]; state[FS_ECUR] = dec[FD_E]; state[FS_P] = dec[FD_P]; state[FS_VV] = dec[FD_VV]; state[FS_FF] = dec[FD_FF];
    state[FS_DTV] = dtv; state[FS_NUPHILL] = dec[FD_NUPHILL]; state[FS_VMAX] = vmax;
    if (limited) state[FS_NLIMITED] += 1.0;
    if (dec[FD_ITER] == 1.0) { state[FS_EFIRST] = dec[FD_E]; state[FS_FFFIRST] = dec[FD_FF]; }
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
  for (int k = 0; k < FS_N; k++) out[1 + k] = state[k];
}

// ---- bond constraints in the RATTLE form (include/ani_md.h, ani_md_shake_positions / ani_md_rattle_velocities) --------------
// One thread per cluster (a centre and K <= 3 partners), everything in registers: the K unknowns of a cluster couple only through
// its centre, so the K x K system is solved directly.  Slots that a cluster does not use are carried as rows and columns of the
// identity with a zero right-hand side: one 3 x 3 solve serves K = 1, 2 and 3, and the unused unknowns stay exactly zero.
static_assert(ANI_MD_SHAKE_NSTATS == 4, "stats layout of include/ani_md.h");

__device__ __forceinline__ double minimg1(double a, double L, int periodic) { return periodic ? a - L * rint(a / L) : a; }

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

// ---- Nose-Hoover chain and thermo record (include/ani_md.h, ani_md_nh_* / ani_md_thermo) ------------------------------------
// Sums as FIRE's: per-block partials with block_sum_fixed, then one workgroup that strides over the partials and sums its 256
// accumulators with block_sum_fixed again.  The chain itself is a few dozen flops on one thread.
enum { NS_COUNT = 0, NS_K2, NS_S, NS_TTARGET, NS_ECOUPLE, NS_TDOF, NS_NONFINITE, NS_ZERO, NS_ETA = 8, NS_ETADOT = 16, NS_ETADOTDOT = 24,
       NS_N = 32 };
static_assert(NS_N == ANI_MD_NH_NSTATE && NS_ETADOT - NS_ETA == ANI_MD_NH_MAXCHAIN, "state layout of include/ani_md.h");
constexpr double NH_BOLTZ = 0.0019872067, NH_MVV2E = 48.88821291 * 48.88821291, NH_NKTV2P = 68568.415;

// m |v|^2 mvv2e of one atom, the multiply-adds spelled out: the same bits wherever it is inlined
__device__ __forceinline__ double k2_term(double m, double v0, double v1, double v2) {
  return (m * fma(v2, v2, fma(v1, v1, v0 * v0))) * NH_MVV2E;
}

__global__ __launch_bounds__(256) void nh_kinetic_kernel(const double* __restrict__ v, const double* __restrict__ mass, int n,
                                                         double* __restrict__ part) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double k2 = 0.0;
  if (i < n) k2 = k2_term(mass[i], v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2]);
  k2 = block_sum_fixed(k2, red);
  if (threadIdx.x == 0) part[blockIdx.x] = k2;
}

// The chain's half-step of include/ani_md.h on one thread: K2 is scaled in place, s and ecouple come back, eta / ed / edd are the
// chain's links in registers (chain_load / the caller's stores).  The thermostat chain and the barostat chain are this one function.
// kt = k_B t_target and ket = tdof kt come rounded from the host: formed here, K2 - tdof kt would contract into one multiply-add
// and a chain at rest exactly on target would start to move.
__device__ __forceinline__ void chain_load(const double* __restrict__ links, int M, double (&eta)[ANI_MD_NH_MAXCHAIN],
                                           double (&ed)[ANI_MD_NH_MAXCHAIN + 1], double (&edd)[ANI_MD_NH_MAXCHAIN]) {
#pragma unroll
  for (int k = 0; k < ANI_MD_NH_MAXCHAIN; k++) {
    const bool used = k < M;
    eta[k] = used ? links[k] : 0.0;
    ed[k] = used ? links[ANI_MD_NH_MAXCHAIN + k] : 0.0;
    edd[k] = used ? links[2 * ANI_MD_NH_MAXCHAIN + k] : 0.0;
  }
  ed[ANI_MD_NH_MAXCHAIN] = 0.0;
}
__device__ __forceinline__ void chain_half_step(double& K2, double kt, double ket, double t_period, double drag, double dt, int M,
                                                int nc, double (&eta)[ANI_MD_NH_MAXCHAIN], double (&ed)[ANI_MD_NH_MAXCHAIN + 1],
                                                double (&edd)[ANI_MD_NH_MAXCHAIN], double& s_out, double& ec_out) {
  double Q[ANI_MD_NH_MAXCHAIN];
  const double tf = 1.0 / t_period;
#pragma unroll
  for (int k = 0; k < ANI_MD_NH_MAXCHAIN; k++) Q[k] = (k == 0 ? ket : kt) / (tf * tf);
  const double nf = 1.0 / (double)nc, dfac = 1.0 - dt * drag / (double)nc;
  const double h2 = nf * dt / 2.0, h4 = nf * dt / 4.0, h8 = nf * dt / 8.0;
  edd[0] = (K2 - ket) / Q[0];
  double s = 1.0;
  for (int it = 0; it < nc; it++) {
    for (int k = M - 1; k >= 1; k--) {
      const double e = exp(-h8 * ed[k + 1]);
      ed[k] = ((ed[k] * e + edd[k] * h4) * dfac) * e;
    }
    const double e0 = exp(-h8 * ed[1]);
    ed[0] = ((ed[0] * e0 + edd[0] * h4) * dfac) * e0;
    const double fac = exp(-h2 * ed[0]);
    s *= fac;
    K2 *= fac * fac;
    edd[0] = (K2 - ket) / Q[0];
    for (int k = 0; k < M; k++) eta[k] += h2 * ed[k];
    ed[0] = (ed[0] * e0 + edd[0] * h4) * e0;
    for (int k = 1; k < M; k++) {
      const double e = exp(-h8 * ed[k + 1]);
      ed[k] *= e;
      edd[k] = (Q[k - 1] * ed[k - 1] * ed[k - 1] - kt) / Q[k];
      ed[k] = (ed[k] + edd[k] * h4) * e;
    }
  }
  double ec = ket * eta[0] + 0.5 * Q[0] * ed[0] * ed[0];
  for (int k = 1; k < M; k++) ec += kt * eta[k] + 0.5 * Q[k] * ed[k] * ed[k];
  s_out = s;
  ec_out = ec;
}

__global__ __launch_bounds__(256) void nh_chain_kernel(double* __restrict__ state, const double* __restrict__ part, int npart,
                                                       double t_target, double tdof, double kt, double ket,
                                                       ani_md_nh_params p) {
  __shared__ double red[4];
  double K2 = 0.0;
  for (int b = threadIdx.x; b < npart; b += 256) K2 += part[b];
  K2 = block_sum_fixed(K2, red);
  if (threadIdx.x != 0) return;
  if (npart == 0) K2 = state[NS_K2];
  state[NS_TTARGET] = t_target;
  state[NS_TDOF] = tdof;
  state[NS_ZERO] = 0.0;
  if (!finite_d(K2)) {
    state[NS_K2] = K2;
    state[NS_S] = 1.0;
    state[NS_NONFINITE] += 1.0;
    return;
  }
  double eta[ANI_MD_NH_MAXCHAIN], ed[ANI_MD_NH_MAXCHAIN + 1], edd[ANI_MD_NH_MAXCHAIN];
  chain_load(state + NS_ETA, p.mtchain, eta, ed, edd);
  double s, ec;
  chain_half_step(K2, kt, ket, p.t_period, p.drag, p.dt, p.mtchain, p.nc_tchain, eta, ed, edd, s, ec);
  state[NS_COUNT] += 1.0;
  state[NS_K2] = K2;
  state[NS_S] = s;
  state[NS_ECOUPLE] = ec;
#pragma unroll
  for (int k = 0; k < ANI_MD_NH_MAXCHAIN; k++) {
    state[NS_ETA + k] = eta[k];
    state[NS_ETADOT + k] = ed[k];
    state[NS_ETADOTDOT + k] = edd[k];
  }
}

__global__ __launch_bounds__(256) void nh_scale_kernel(double* __restrict__ v, int n, const double* __restrict__ state) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < 3 * n) v[t] *= state[NS_S];
}

// initial_integrate_kernel with v = s v in front of it
__global__ __launch_bounds__(256) void nh_initial_integrate_kernel(double* __restrict__ x, double* __restrict__ v,
                                                                   const double* __restrict__ f, const double* __restrict__ dtfm,
                                                                   double dt, int n, const double* __restrict__ xb,
                                                                   double* __restrict__ d2max, const double* __restrict__ state) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double d2 = 0.0;
  if (i < n) {
    const double s = dtfm[i], sc = state[NS_S];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double vk = fma(s, f[3 * i + k], sc * v[3 * i + k]);   // s v rounded, then the kick as initial_integrate_kernel contracts it
      const double xk = x[3 * i + k] + dt * vk;
      v[3 * i + k] = vk;
      x[3 * i + k] = xk;
      const double d = xk - xb[3 * i + k];
      d2 += d * d;
    }
  }
  __shared__ double red[4];
  d2 = block_max(d2, red);
  if (threadIdx.x == 0) raise_d2max(d2, d2max);
}

// final_integrate_kernel without the thermostat term, and nh_kinetic_kernel on what it wrote
__global__ __launch_bounds__(256) void nh_final_integrate_kernel(double* __restrict__ v, const double* __restrict__ f,
                                                                 const double* __restrict__ dtfm, const double* __restrict__ mass,
                                                                 int n, double* __restrict__ part) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double k2 = 0.0;
  if (i < n) {
    const double s = dtfm[i];
    double vn[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      vn[k] = v[3 * (size_t)i + k] + s * f[3 * (size_t)i + k];
      v[3 * (size_t)i + k] = vn[k];
    }
    k2 = k2_term(mass[i], vn[0], vn[1], vn[2]);
  }
  k2 = block_sum_fixed(k2, red);
  if (threadIdx.x == 0) part[blockIdx.x] = k2;
}

// ---- isotropic barostat (include/ani_md.h, ani_md_npt_*) --------------------------------------------------------------------
// The box is six doubles of the barostat record; one thread of one workgroup moves it, the per-atom kernels read mu, fv, c and the
// shift ratio from the record.  Everything a half-step decides is formed in registers first and written only when K2, Wtr and the
// new strain rate are finite.
enum { PS_COUNT = 0, PS_WD, PS_OMEGA, PS_P, PS_PTARGET, PS_W, PS_FV, PS_MU, PS_LO = 8, PS_LEN = 11, PS_RATIO = 14, PS_C = 17, PS_V0 = 20,
       PS_ECOUPLE, PS_NONFINITE, PS_NATOMS, PS_ETA = 24, PS_ETADOT = 32, PS_ETADOTDOT = 40, PS_ECHAIN = 48, PS_VOL, PS_N = 56 };
static_assert(PS_N == ANI_MD_NPT_NSTATE && PS_ETADOT - PS_ETA == ANI_MD_NH_MAXCHAIN && PS_ETADOTDOT - PS_ETADOT == ANI_MD_NH_MAXCHAIN,
              "barostat record layout of include/ani_md.h");

__global__ void npt_init_kernel(double* __restrict__ ps, double lo0, double lo1, double lo2, double l0, double l1, double l2, double n) {
  for (int k = 0; k < PS_N; k++) ps[k] = 0.0;
  const double lo[3] = {lo0, lo1, lo2}, len[3] = {l0, l1, l2};
  for (int k = 0; k < 3; k++) {
    ps[PS_LO + k] = lo[k];
    ps[PS_LEN + k] = len[k];
    ps[PS_RATIO + k] = 1.0;
    ps[PS_C + k] = lo[k] + 0.5 * len[k];
  }
  const double V = (l0 * l1) * l2;
  ps[PS_FV] = 1.0;
  ps[PS_MU] = 1.0;
  ps[PS_V0] = V;
  ps[PS_VOL] = V;
  ps[PS_NATOMS] = n;
}

__global__ __launch_bounds__(256) void npt_chain_kernel(int phase, double* __restrict__ ns, double* __restrict__ ps,
                                                        const double* __restrict__ part, int npart, const double* __restrict__ ev,
                                                        double t_target, double p_target, double tdof, double kt, double ket,
                                                        ani_md_npt_params p) {
  __shared__ double red[4];
  double K2 = 0.0;
  for (int b = threadIdx.x; b < npart; b += 256) K2 += part[b];
  K2 = block_sum_fixed(K2, red);
  if (threadIdx.x != 0) return;
  if (npart == 0) K2 = ns[NS_K2];
  const double K2_in = K2;
  const double Wtr = (ev[1] + ev[5]) + ev[9];
  const double N = ps[PS_NATOMS];
  const double W = ((N + 1.0) * kt) * (p.p_period * p.p_period);
  double lo[3], len[3], c[3];
  for (int k = 0; k < 3; k++) { lo[k] = ps[PS_LO + k]; len[k] = ps[PS_LEN + k]; c[k] = ps[PS_C + k]; }
  const double V = (len[0] * len[1]) * len[2];
  double wd = ps[PS_WD];
  double eta[ANI_MD_NH_MAXCHAIN], ed[ANI_MD_NH_MAXCHAIN + 1], edd[ANI_MD_NH_MAXCHAIN];
  double peta[ANI_MD_NH_MAXCHAIN], ped[ANI_MD_NH_MAXCHAIN + 1], pedd[ANI_MD_NH_MAXCHAIN];
  chain_load(ns + NS_ETA, p.mtchain, eta, ed, edd);
  chain_load(ps + PS_ETA, p.mpchain, peta, ped, pedd);
  double s = 1.0, ec = 0.0, sb = 1.0, ecb = 0.0, P = 0.0;
  const double hdt = 0.5 * p.dt;
  if (phase == 0) {
    double Kb = (W * wd) * wd;
    chain_half_step(Kb, kt, kt, p.p_period, 0.0, p.dt, p.mpchain, p.nc_pchain, peta, ped, pedd, sb, ecb);
    wd *= sb;
    chain_half_step(K2, kt, ket, p.t_period, p.drag, p.dt, p.mtchain, p.nc_tchain, eta, ed, edd, s, ec);
  }
  {
    P = (K2 + Wtr) / (3.0 * V) * NH_NKTV2P;
    const double a = (P - p_target) * V / NH_NKTV2P, b = K2 / (3.0 * N);
    wd += hdt * ((a + b) / W);
  }
  if (phase != 0) {
    chain_half_step(K2, kt, ket, p.t_period, p.drag, p.dt, p.mtchain, p.nc_tchain, eta, ed, edd, s, ec);
    double Kb = (W * wd) * wd;
    chain_half_step(Kb, kt, kt, p.p_period, 0.0, p.dt, p.mpchain, p.nc_pchain, peta, ped, pedd, sb, ecb);
    wd *= sb;
  }
  ns[NS_TTARGET] = t_target;
  ns[NS_TDOF] = tdof;
  ns[NS_ZERO] = 0.0;
  ps[PS_PTARGET] = p_target;
  if (!(finite_d(K2_in) && finite_d(Wtr) && finite_d(wd))) {
    ns[NS_K2] = K2_in;
    ns[NS_S] = 1.0;
    ns[NS_NONFINITE] += 1.0;
    ps[PS_FV] = 1.0;
    ps[PS_MU] = 1.0;
    for (int k = 0; k < 3; k++) ps[PS_RATIO + k] = 1.0;
    ps[PS_NONFINITE] += 1.0;
    return;
  }
  double Vnew = V;
  if (phase == 0) {
    const double fv = exp(-hdt * (wd * (1.0 + 1.0 / N))), mu = exp(hdt * wd), mu2 = mu * mu;
    ps[PS_FV] = fv;
    ps[PS_MU] = mu;
    double ln[3];
    for (int k = 0; k < 3; k++) {
      ln[k] = len[k] * mu2;
      const double d = lo[k] - c[k];
      ps[PS_LO + k] = c[k] + mu2 * d;
      ps[PS_LEN + k] = ln[k];
      ps[PS_RATIO + k] = ln[k] / len[k];
    }
    Vnew = (ln[0] * ln[1]) * ln[2];
    ps[PS_OMEGA] += p.dt * wd;
  }
  ns[NS_COUNT] += 1.0;
  ns[NS_K2] = K2;
  ns[NS_S] = s;
  ns[NS_ECOUPLE] = ec;
  ps[PS_COUNT] += 1.0;
  ps[PS_WD] = wd;
  ps[PS_P] = P;
  ps[PS_W] = W;
  ps[PS_VOL] = Vnew;
  ps[PS_ECHAIN] = ecb;
  ps[PS_ECOUPLE] = 3.0 * (0.5 * W * wd * wd + ecb) + p_target * (Vnew - ps[PS_V0]) / NH_NKTV2P;
#pragma unroll
  for (int k = 0; k < ANI_MD_NH_MAXCHAIN; k++) {
    ns[NS_ETA + k] = eta[k];
    ns[NS_ETADOT + k] = ed[k];
    ns[NS_ETADOTDOT + k] = edd[k];
    ps[PS_ETA + k] = peta[k];
    ps[PS_ETADOT + k] = ped[k];
    ps[PS_ETADOTDOT + k] = pedd[k];
  }
}

// step 5 of the first half on the owned rows, step 7 on the shift rows behind them: one grid over n + nghost rows
__global__ __launch_bounds__(256) void npt_initial_integrate_kernel(double* __restrict__ x, double* __restrict__ v,
                                                                    const double* __restrict__ f, const double* __restrict__ dtfm,
                                                                    double dt, int n, const double* __restrict__ xb,
                                                                    double* __restrict__ d2max, const double* __restrict__ ns,
                                                                    const double* __restrict__ ps, double* __restrict__ shift,
                                                                    int nghost) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double d2 = 0.0;
  if (i < n) {
    const double s = dtfm[i], sc = ns[NS_S] * ps[PS_FV], mu = ps[PS_MU];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const size_t e = 3 * (size_t)i + k;
      const double c = ps[PS_C + k];
      const double vk = sc * v[e] + s * f[e];
      double xk = c + mu * (x[e] - c);
      xk = xk + dt * vk;
      xk = c + mu * (xk - c);
      v[e] = vk;
      x[e] = xk;
      const double d = xk - xb[e];
      d2 += d * d;
    }
  } else if (i - n < nghost) {
    const size_t g = 3 * (size_t)(i - n);
#pragma unroll
    for (int k = 0; k < 3; k++) shift[g + k] *= ps[PS_RATIO + k];
  }
  __shared__ double red[4];
  d2 = block_max(d2, red);
  if (threadIdx.x == 0 && blockIdx.x * blockDim.x < n) raise_d2max(d2, d2max);
}

// nh_final_integrate_kernel with v *= fv behind the kick; the partials are nh_kinetic_kernel's on what it wrote
__global__ __launch_bounds__(256) void npt_final_integrate_kernel(double* __restrict__ v, const double* __restrict__ f,
                                                                  const double* __restrict__ dtfm, const double* __restrict__ mass,
                                                                  int n, const double* __restrict__ ps, double* __restrict__ part) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double k2 = 0.0;
  if (i < n) {
    const double s = dtfm[i], fv = ps[PS_FV];
    double vn[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      vn[k] = (v[3 * (size_t)i + k] + s * f[3 * (size_t)i + k]) * fv;
      v[3 * (size_t)i + k] = vn[k];
    }
    k2 = k2_term(mass[i], vn[0], vn[1], vn[2]);
  }
  k2 = block_sum_fixed(k2, red);
  if (threadIdx.x == 0) part[blockIdx.x] = k2;
}

__global__ void npt_check_kernel(double* __restrict__ d2max, const double* __restrict__ ev, const double* __restrict__ ps,
                                 double* __restrict__ out) {
  const double e = ev[0];
  out[0] = finite_d(e) ? d2max[0] : __longlong_as_double(0x7ff0000000000000LL);
  d2max[0] = 0.0;
  for (int k = 0; k < PS_N; k++) out[1 + k] = ps[k];
}

// part[c nblk + b] = K_c of block b, c = xx, yy, zz, xy, xz, yz
__global__ __launch_bounds__(256) void thermo_reduce_kernel(const double* __restrict__ v, const double* __restrict__ mass, int n,
                                                            double* __restrict__ part) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x, nblk = gridDim.x;
  double k[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < n) {
    const double m = mass[i], v0 = v[3 * (size_t)i], v1 = v[3 * (size_t)i + 1], v2 = v[3 * (size_t)i + 2];
    k[0] = (m * v0 * v0) * NH_MVV2E; k[1] = (m * v1 * v1) * NH_MVV2E; k[2] = (m * v2 * v2) * NH_MVV2E;
    k[3] = (m * v0 * v1) * NH_MVV2E; k[4] = (m * v0 * v2) * NH_MVV2E; k[5] = (m * v1 * v2) * NH_MVV2E;
  }
#pragma unroll
  for (int c = 0; c < 6; c++) {
    const double sum = block_sum_fixed(k[c], red);
    if (threadIdx.x == 0) part[c * nblk + blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(256) void thermo_finish_kernel(const double* __restrict__ part, int nblk, const double* __restrict__ ev,
                                                            int with_virial, double tdof, double volume,
                                                            const double* __restrict__ nh_state, double* __restrict__ out) {
  __shared__ double red[4];
  double K[6];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    double a = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) a += part[c * nblk + b];
    K[c] = block_sum_fixed(a, red);
  }
  if (threadIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double k2 = (K[0] + K[1]) + K[2], ke = 0.5 * k2, pe = ev[0];
  const double ec = nh_state ? nh_state[NS_ECOUPLE] : 0.0;
  out[0] = pe;
  out[1] = ke;
  out[2] = 2.0 * ke / (tdof * NH_BOLTZ);
  // W_ab = ev[1 + 3 a + b]: xx, yy, zz at 1, 5, 9; xy, xz, yz at 2, 3, 6
  const int wi[6] = {1, 5, 9, 2, 3, 6};
  out[3] = with_virial ? (k2 + ((ev[1] + ev[5]) + ev[9])) / (3.0 * volume) * NH_NKTV2P : nan;
#pragma unroll
  for (int c = 0; c < 6; c++) out[4 + c] = with_virial ? (K[c] + ev[wi[c]]) / volume * NH_NKTV2P : nan;
  out[10] = pe + ke;
  out[11] = ec;
  out[12] = (pe + ke) + ec;
  out[13] = volume;
  out[14] = k2;
  out[15] = 0.0;
}

// ---- umbrella restraints on collective variables (include/ani_md.h, ani_md_restraints_eval / ani_md_restraints_apply) --------
// Two launches behind the force evaluation.  eval: one thread per restraint, everything in registers, writes only its own rows of
// cv, e, fslot and w -- restraints share atoms, so nothing is added into f here.  apply: one thread per touched atom walks the
// host-built gather table in its fixed order (no floating-point atomics), and one further workgroup sums e and w in the fixed
// order of the sums above and writes ev, the record and the series row.
static_assert(ANI_MD_RESTRAINT_NREC == 16, "record layout of include/ani_md.h");

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
  rec[0] += 1.0;
  rec[1] = E;
#pragma unroll
  for (int c = 0; c < 9; c++) rec[2 + c] = W[c];
  rec[11] = bad;
  rec[12] = dmax;
  rec[13] = skipped;
  rec[14] = rec[15] = 0.0;
  if (series_row) series_row[0] = step;
}

// ---- launches ---------------------------------------------------------------------------------------------------------------
// everything goes on the caller's stream; blocks(count) workgroups of 256 threads unless an entry point says otherwise
inline dim3 blocks(int count) { return dim3((count + 255) / 256); }
inline int nblocks(int nlocal) { return nlocal > 0 ? (nlocal + 255) / 256 : 1; }
inline const long long* ll(const int64_t* p) { return reinterpret_cast<const long long*>(p); }
inline long long* ll(int64_t* p) { return reinterpret_cast<long long*>(p); }

template <typename K, typename... A>
void enqueue(K kernel, dim3 grid, int block, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, grid, dim3(block), 0, (hipStream_t)stream, args...);
}
template <typename K, typename... A>
int launch(K kernel, dim3 grid, int block, void* stream, A... args) {
  enqueue(kernel, grid, block, stream, args...);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ani_md_gather_rows(const double* src, const int64_t* idx, int n, double* out, void* stream) {
  if (n <= 0) return 0;
  return launch(gather_rows_kernel, blocks(3 * n), 256, stream, src, ll(idx), n, out);
}

int ani_md_scatter_rows(double* dst, const int64_t* idx, int n, const double* in, void* stream) {
  if (n <= 0) return 0;
  return launch(scatter_rows_kernel, blocks(3 * n), 256, stream, dst, ll(idx), n, in);
}

int ani_md_initial_integrate(double* x, double* v, const double* f, const double* dtfm, double dt, int nlocal,
                             const double* x_built, double* d2max, void* stream) {
  if (nlocal <= 0) return 0;
  return launch(initial_integrate_kernel, blocks(nlocal), 256, stream, x, v, f, dtfm, dt, nlocal, x_built, d2max);
}

int ani_md_final_integrate(double* v, double* f, const double* dtfm, int nlocal, int langevin, const double* g1,
                           const double* g2, const int64_t* tag, uint64_t seed, uint64_t step, void* stream) {
  if (nlocal <= 0) return 0;
  return launch(final_integrate_kernel, blocks(nlocal), 256, stream, v, f, dtfm, nlocal, langevin, g1, g2, ll(tag),
                (unsigned long long)seed, (unsigned long long)step);
}

int ani_md_final_initial_integrate(double* x, double* v, double* f, const double* dtfm, double dt, int nlocal, int langevin,
                                   const double* g1, const double* g2, const int64_t* tag, uint64_t seed, uint64_t step,
                                   const double* x_built, double* d2max, void* stream) {
  if (nlocal <= 0) return 0;
  return launch(final_initial_integrate_kernel, blocks(nlocal), 256, stream, x, v, f, dtfm, dt, nlocal, langevin, g1, g2, ll(tag),
                (unsigned long long)seed, (unsigned long long)step, x_built, d2max);
}

int ani_md_forward_ghosts(double* x, const int64_t* owner, const double* shift, int nlocal, int nghost, void* stream) {
  if (nghost <= 0) return 0;
  return launch(forward_ghosts_kernel, blocks(3 * nghost), 256, stream, x, ll(owner), shift, nlocal, nghost);
}

int ani_md_reverse_ghosts(double* f, const int64_t* owner, int nlocal, int nghost, void* stream) {
  if (nghost <= 0) return 0;
  return launch(reverse_ghosts_kernel, blocks(3 * nghost), 256, stream, f, ll(owner), nlocal, nghost);
}

int ani_md_reverse_ghosts_ordered(double* f, const int64_t* owner, const int64_t* ghost_of, int nlocal, int nghost, void* stream) {
  if (nghost <= 0) return 0;
  if (!ghost_of) return ani_md_reverse_ghosts(f, owner, nlocal, nghost, stream);
  return launch(reverse_ghosts_ordered_kernel, blocks(3 * nghost), 256, stream, f, ll(owner), ll(ghost_of), nlocal, nghost);
}

int ani_md_pack_ghosts(const double* x, const int64_t* owner, const double* shift, int nsend, double* out, void* stream) {
  if (nsend <= 0) return 0;
  return launch(pack_ghosts_kernel, blocks(3 * nsend), 256, stream, x, ll(owner), shift, nsend, out);
}

int ani_md_unpack_reverse(double* f, const int64_t* owner, int nsend, const double* in, void* stream) {
  if (nsend <= 0) return 0;
  return launch(unpack_reverse_kernel, blocks(3 * nsend), 256, stream, f, ll(owner), nsend, in);
}

int ani_md_wrap_positions(double* x, int n, const double* lo3, const double* len3, int periodic_mask, void* stream) {
  if (n <= 0 || !periodic_mask) return 0;
  return launch(wrap_kernel, blocks(3 * n), 256, stream, x, n, lo3[0], lo3[1], lo3[2], len3[0], len3[1], len3[2], periodic_mask);
}

int ani_md_ghost_shell_count(const double* x, int n, const double* clo, const double* chi, int ncombo, int* blk_cnt, int* blk_off,
                             int* out_counts, void* stream) {
  if (ncombo <= 0) return 0;
  const int nblk = nblocks(n);
  enqueue(shell_count_kernel, dim3(nblk, ncombo), 256, stream, x, n, clo, chi, nblk, blk_cnt);
  return launch(shell_scan_kernel, dim3(1), 1024, stream, blk_cnt, blk_off, ncombo, nblk, out_counts);
}

int ani_md_ghost_shell_fill(const double* x, int n, const double* clo, const double* chi, const double* cshift, int ncombo,
                            const int* blk_off, int64_t* send_idx, double* send_shift, void* stream) {
  if (ncombo <= 0) return 0;
  const int nblk = nblocks(n);
  return launch(shell_fill_kernel, dim3(nblk, ncombo), 256, stream, x, n, clo, chi, cshift, nblk, blk_off, ll(send_idx), send_shift);
}

int ani_md_append_ghosts(double* x, int* species, int nlocal, const int64_t* owner, const double* shift, int nghost, void* stream) {
  if (nghost <= 0) return 0;
  return launch(append_ghosts_kernel, blocks(nghost), 256, stream, x, species, nlocal, ll(owner), shift, nghost);
}

int ani_md_check(double* d2max, const double* ev, double* out, void* stream) {
  return launch(check_kernel, dim3(1), 1, stream, d2max, ev, out);
}

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

int ani_md_nh_work_size(int nlocal) { return nblocks(nlocal); }

int ani_md_nh_init(double* state, void* stream) {
  if (!state) return (int)hipErrorInvalidValue;
  return (int)hipMemsetAsync(state, 0, sizeof(double) * ANI_MD_NH_NSTATE, (hipStream_t)stream);
}

int ani_md_nh_kinetic(const double* v, const double* mass, int nlocal, double* work, void* stream) {
  if (nlocal <= 0) return 0;
  if (!v || !mass || !work) return (int)hipErrorInvalidValue;
  return launch(nh_kinetic_kernel, blocks(nlocal), 256, stream, v, mass, nlocal, work);
}

int ani_md_nh_chain(double* state, const double* work, int npart, double t_target, double tdof, const ani_md_nh_params* params,
                    void* stream) {
  if (!state || !params || npart < 0 || (npart > 0 && !work)) return (int)hipErrorInvalidValue;
  if (params->mtchain < 1 || params->mtchain > ANI_MD_NH_MAXCHAIN || params->nc_tchain < 1 || !(params->t_period > 0.0) ||
      !(params->dt > 0.0) || !(t_target > 0.0) || !(tdof > 0.0))
    return (int)hipErrorInvalidValue;
  const double kt = 0.0019872067 * t_target, ket = tdof * kt;
  return launch(nh_chain_kernel, dim3(1), 256, stream, state, work, npart, t_target, tdof, kt, ket, *params);
}

int ani_md_nh_scale(double* v, int nlocal, const double* state, void* stream) {
  if (nlocal <= 0) return 0;
  if (!v || !state) return (int)hipErrorInvalidValue;
  return launch(nh_scale_kernel, blocks(3 * nlocal), 256, stream, v, nlocal, state);
}

int ani_md_nh_initial_integrate(double* x, double* v, const double* f, const double* dtfm, double dt, int nlocal,
                                const double* x_built, double* d2max, const double* state, void* stream) {
  if (nlocal <= 0) return 0;
  if (!state) return (int)hipErrorInvalidValue;
  return launch(nh_initial_integrate_kernel, blocks(nlocal), 256, stream, x, v, f, dtfm, dt, nlocal, x_built, d2max, state);
}

int ani_md_nh_final_integrate(double* v, const double* f, const double* dtfm, const double* mass, int nlocal, double* work,
                              void* stream) {
  if (nlocal <= 0) return 0;
  if (!mass || !work) return (int)hipErrorInvalidValue;
  return launch(nh_final_integrate_kernel, blocks(nlocal), 256, stream, v, f, dtfm, mass, nlocal, work);
}

int ani_md_npt_init(double* npt_state, const double* lo3, const double* len3, int nlocal, void* stream) {
  if (!npt_state || !lo3 || !len3 || nlocal <= 0) return (int)hipErrorInvalidValue;
  for (int k = 0; k < 3; k++)
    if (!(len3[k] > 0.0) || !(len3[k] - len3[k] == 0.0) || !(lo3[k] - lo3[k] == 0.0)) return (int)hipErrorInvalidValue;
  return launch(npt_init_kernel, dim3(1), 1, stream, npt_state, lo3[0], lo3[1], lo3[2], len3[0], len3[1], len3[2], (double)nlocal);
}

int ani_md_npt_chain(int phase, double* nh_state, double* npt_state, const double* work, int npart, const double* ev, double t_target,
                     double p_target, double tdof, const ani_md_npt_params* params, void* stream) {
  if (!nh_state || !npt_state || !ev || !params || npart < 0 || (npart > 0 && !work) || (phase != 0 && phase != 1))
    return (int)hipErrorInvalidValue;
  const ani_md_npt_params& q = *params;
  if (q.mtchain < 1 || q.mtchain > ANI_MD_NH_MAXCHAIN || q.mpchain < 1 || q.mpchain > ANI_MD_NH_MAXCHAIN || q.nc_tchain < 1 ||
      q.nc_pchain < 1 || !(q.t_period > 0.0) || !(q.p_period > 0.0) || !(q.dt > 0.0) || !(t_target > 0.0) || !(tdof > 0.0) ||
      !(p_target - p_target == 0.0))
    return (int)hipErrorInvalidValue;
  const double kt = 0.0019872067 * t_target, ket = tdof * kt;
  return launch(npt_chain_kernel, dim3(1), 256, stream, phase, nh_state, npt_state, work, npart, ev, t_target, p_target, tdof, kt, ket, q);
}

int ani_md_npt_initial_integrate(double* x, double* v, const double* f, const double* dtfm, double dt, int nlocal,
                                 const double* x_built, double* d2max, const double* nh_state, const double* npt_state,
                                 double* shift, int nghost, void* stream) {
  if (nghost < 0) return (int)hipErrorInvalidValue;
  if (nlocal <= 0) return 0;
  if (!nh_state || !npt_state || (nghost > 0 && !shift)) return (int)hipErrorInvalidValue;
  return launch(npt_initial_integrate_kernel, blocks(nlocal + nghost), 256, stream, x, v, f, dtfm, dt, nlocal, x_built, d2max, nh_state,
                npt_state, shift, nghost);
}

int ani_md_npt_final_integrate(double* v, const double* f, const double* dtfm, const double* mass, int nlocal,
                               const double* npt_state, double* work, void* stream) {
  if (nlocal <= 0) return 0;
  if (!mass || !work || !npt_state) return (int)hipErrorInvalidValue;
  return launch(npt_final_integrate_kernel, blocks(nlocal), 256, stream, v, f, dtfm, mass, nlocal, npt_state, work);
}

int ani_md_npt_check(double* d2max, const double* ev, const double* npt_state, double* out, void* stream) {
  if (!npt_state) return (int)hipErrorInvalidValue;
  return launch(npt_check_kernel, dim3(1), 1, stream, d2max, ev, npt_state, out);
}

int ani_md_thermo_work_size(int nlocal) { return 6 * nblocks(nlocal); }

int ani_md_thermo(const double* v, const double* mass, int nlocal, const double* ev, int with_virial, double tdof, double volume,
                  const double* nh_state, double* work, double* out, void* stream) {
  if (!ev || !out || (nlocal > 0 && (!v || !mass || !work))) return (int)hipErrorInvalidValue;
  const int nblk = nlocal > 0 ? (nlocal + 255) / 256 : 0;
  if (nblk) enqueue(thermo_reduce_kernel, dim3(nblk), 256, stream, v, mass, nlocal, work);
  return launch(thermo_finish_kernel, dim3(1), 256, stream, work, nblk, ev, with_virial, tdof, volume, nh_state, out);
}

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
