// ani_kernels_md.hip — the timestep loop's own kernels (include/ani_md.h): what LAMMPS' fix nve, fix langevin,
// Neighbor::check_distance and Comm do around PairANI::compute in the reference's runs
// (examples/benchmark/in.lammps:24-27,54-72).  Test / bench infrastructure of the LAMMPS-free loop, not the pair style.
#include "ani_md_device.h"

namespace {

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
      d2 += drift_d2(x, v, xb, 3 * i + k, dt, vk);
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
      d2 += drift_d2(x, v, xb, 3 * i + k, dt, vk);
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

}  // extern "C"
