// ani_kernels_rdf.hip — radial distribution functions over the installed neighbour list (ani_rdf_*, include/ani_hip.h).
//
// What LAMMPS' `compute rdf` + `fix ave/time` give the reference's runs, done on the list the step already keeps: every pair
// inside the force cutoff is in it.  One launch per frame:
//
//   rdf_accumulate  LANES lanes per centre (16, or a whole wave) walk its list segment, dense or capacity row alike.  An entry
//                   is rejected on the ordered species pair first (slot_of), then r = |x_j - x_i| in fp64 from the caller's
//                   doubles, k = (int)(r * inv_dr), counted in hist[slot][k] when r < rmax and k < nbins.
//
// A workgroup counts into a private histogram of 32-bit words in LDS, runs over centres in a grid-stride loop and adds its
// non-zero bins into the global 64-bit words at the end: one flush per workgroup, at most kRdfMaxBlocks of them.  A workgroup
// sees fewer than 2^31 list entries (jlist is indexed by int), so a 32-bit word cannot wrap.  Above kRdfLdsBins bins the same
// kernel counts straight into the global words.  The valid centres of every species are counted per wave (a ballot per species),
// folded into LDS once per wave and into centres[p] once per workgroup and pair; one thread bumps frames.
//
// Integer atomics only: counts are exact and independent of the schedule.  No lane, wave or workgroup waits for another; the
// accumulators are written by atomics alone and read after the launch, by a copy on the same stream.
#include <algorithm>

#include "ani_kernels.h"

namespace ani {

namespace {

template <int LANES, bool LDS>
__global__ __launch_bounds__(256) void rdf_accumulate_kernel(RdfArgs a) {
  static_assert(LANES == 16 || LANES == 64, "a centre's lanes lie inside one wave");
  __shared__ unsigned lh[LDS ? kRdfLdsBins : 1];
  __shared__ int lslot[kMaxSpecies * kMaxSpecies];
  __shared__ unsigned lcent[kMaxSpecies];
  const int S = a.S, nh = a.npair * a.nbins;
  if (LDS)
    for (int t = threadIdx.x; t < nh; t += 256) lh[t] = 0;
  for (int t = threadIdx.x; t < S * S; t += 256) lslot[t] = a.slot_of[t];
  if (threadIdx.x < kMaxSpecies) lcent[threadIdx.x] = 0;
  __syncthreads();
  constexpr int G = 256 / LANES;   // centres of a workgroup per pass
  const int sub = threadIdx.x & (LANES - 1), grp = threadIdx.x / LANES, lane = threadIdx.x & 63;
  unsigned ncentre = 0;            // lane s of a wave: the wave's valid centres of species s
  // the bound is the workgroup's, not the lane's: every wave reaches the ballots below with all its lanes
  for (long long base = (long long)blockIdx.x * G; base < a.nlocal; base += (long long)gridDim.x * G) {
    const long long ii = base + grp;
    int si = -1;
    if (ii < a.nlocal) {
      const int i = a.ilist[ii];
      if ((unsigned)i < (unsigned)a.nlocal) {
        si = a.species[i];
        if ((unsigned)si >= (unsigned)S) si = -1;
      }
      if (si >= 0) {
        const int* srow = lslot + si * S;
        const double xi = a.x[3 * (size_t)i], yi = a.x[3 * (size_t)i + 1], zi = a.x[3 * (size_t)i + 2];
        const int* seg = a.jlist + a.nbr_off[ii];
        const int n = a.numneigh[ii];
        for (int k = sub; k < n; k += LANES) {
          const int j = seg[k];
          if ((unsigned)j >= (unsigned)a.ntotal) continue;
          const int sj = a.species[j];
          if ((unsigned)sj >= (unsigned)S) continue;
          const int slot = srow[sj];
          if (slot < 0) continue;   // not asked for: rejected before the position is loaded
          const double dx = a.x[3 * (size_t)j] - xi, dy = a.x[3 * (size_t)j + 1] - yi, dz = a.x[3 * (size_t)j + 2] - zi;
          const double r = sqrt(dx * dx + dy * dy + dz * dz);
          if (!(r < a.rmax)) continue;
          const int kb = (int)(r * a.inv_dr);
          if (kb >= a.nbins) continue;
          if (LDS) atomicAdd(&lh[slot * a.nbins + kb], 1u);
          else atomicAdd(a.hist + (size_t)slot * a.nbins + kb, 1ull);
        }
      }
    }
    for (int s = 0; s < S; s++) {
      const unsigned long long m = __ballot(sub == 0 && si == s);
      if (lane == s) ncentre += (unsigned)__popcll(m);
    }
  }
  if (lane < S && ncentre) atomicAdd(&lcent[lane], ncentre);
  __syncthreads();
  if (LDS)
    for (int t = threadIdx.x; t < nh; t += 256) {
      const unsigned v = lh[t];
      if (v) atomicAdd(a.hist + t, (unsigned long long)v);
    }
  if ((int)threadIdx.x < a.npair) {
    const unsigned v = lcent[a.pair_a[threadIdx.x]];
    if (v) atomicAdd(a.centres + threadIdx.x, (unsigned long long)v);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.frames, 1ull);
}

template <int LANES>
void rdf_launch(const RdfArgs& a, bool lds, hipStream_t st) {
  const long long want = ((long long)a.nlocal * LANES + 255) / 256;
  const unsigned blocks = (unsigned)std::min<long long>(std::max<long long>(want, 1), kRdfMaxBlocks);
  if (lds) hipLaunchKernelGGL((rdf_accumulate_kernel<LANES, true>), dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((rdf_accumulate_kernel<LANES, false>), dim3(blocks), dim3(256), 0, st, a);
}

}  // namespace

void launch_rdf_accumulate(const RdfArgs& a, int lanes, int use_lds, hipStream_t st) {
  static_assert(kRdfLdsBins * sizeof(unsigned) <= 48 * 1024, "static LDS");
  const bool lds = use_lds && (long long)a.npair * a.nbins <= kRdfLdsBins;
  if (lanes == 64) rdf_launch<64>(a, lds, st);
  else rdf_launch<16>(a, lds, st);
  note_launch_error(hipGetLastError());
}

}  // namespace ani
