// ani_md_device.h — device pieces and launch helpers that the translation units of the timestep loop share (ani_kernels_md*.hip):
// block reductions in a fixed order, the displacement fold, fix langevin's counter-based draws, the minimum image of one
// component, the box of the moment and the unwrapped coordinate.  Everything is internal to the unit that includes it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ani_md.h"

namespace {

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
// the drift of one component e with the new velocity vk, both stored:  v = vk;  x += dt vk;  returns (x - xb)^2 for the fold
__device__ __forceinline__ double drift_d2(double* __restrict__ x, double* __restrict__ v, const double* __restrict__ xb, int e,
                                           double dt, double vk) {
  const double xk = x[e] + dt * vk;
  v[e] = vk;
  x[e] = xk;
  const double d = xk - xb[e];
  return d * d;
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

__device__ __forceinline__ double minimg1(double a, double L, int periodic) { return periodic ? a - L * rint(a / L) : a; }

// the box of the moment: three doubles of the device record when there is one, the host's otherwise
struct Box3 {
  double len[3];
};
__device__ __forceinline__ Box3 box_now(double L0, double L1, double L2, const double* __restrict__ box_dev) {
  Box3 b = {{L0, L1, L2}};
  if (box_dev) { b.len[0] = box_dev[0]; b.len[1] = box_dev[1]; b.len[2] = box_dev[2]; }
  return b;
}

// THE unwrapped coordinate (include/ani_md_transport.h; ani_md_protocol.h takes its centre of mass in it): product and sum rounded
// separately, never contracted into an fma
__device__ __forceinline__ double unwrapped(double x, int image, double L, int periodic) {
#pragma clang fp contract(off)
  if (!periodic) return x;
  const double shift = (double)image * L;
  return x + shift;
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
