// ani_kernels_mol.hip — molecule finder over the installed neighbour list (ani_find_molecules*, include/ani_hip.h).
//
// What the reference does in a second GPU program (examples/combustion/analyze.py: a 2 A neighbour list of a dumped
// trajectory, bonds by a per-element-pair length, cuGraph components, a count per sorted formula) done here on the list the
// step already keeps: every pair that can be a bond is inside the 7.1 A list.  Integer results, canonical labels.
//
//   mol_init     parent[i] = i, marks, compositions, table and counters cleared
//   mol_union    16 lanes per centre walk its list segment: entries rejected on species first, then |x_j - x_i|^2 in fp64
//                against cut^2; an accepted entry unites the centre with the neighbour's owner in `parent`
//   mol_flatten  mol_of_atom[i] = find(i); the atom's species into its root's composition; its open mark into the root
//   mol_tally    one lane per root: summary counts, composition packed into a 64-bit key and counted in an open-addressing
//                table; a composition that does not fit the key goes to a list of its own
//   mol_decode   table slots and listed molecules -> formula rows, each behind a row cursor checked against formula_cap
//   mol_summary  the six numbers
//
// No kernel waits for another lane, wave or workgroup.  The union is the lock-free scheme of ECL-CC (Jaiganesh & Burtscher,
// HPDC 2018): a root is only ever hooked under a SMALLER index (atomicCAS on the root's own word), path halving only replaces
// a non-root's pointer by one of its ancestors, so along every chain the indices strictly decrease: find() ends after at
// most `x` steps whatever other lanes do, and a failed CAS hands back the loser's new, smaller parent, from which the lane
// goes on -- the larger of the two roots a lane holds drops with every failure.  When the launch is over every component
// has one root, its smallest index.  parent[] is read and written with relaxed agent-scope atomics inside the launches that
// change it: a CU's L1 is not refreshed by other CUs' stores, and a plain load could keep returning a root that is none.
#include <algorithm>

#include "ani_kernels.h"

namespace ani {

namespace {

constexpr unsigned long long kMolEmpty = ~0ull;

__device__ __forceinline__ int mol_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mol_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x, with path halving.  Every step moves to a strictly smaller index.
__device__ __forceinline__ int mol_find(int* parent, int x) {
  int cur = x;
  int p = mol_ld(parent + cur);
  while (p != cur) {
    const int gp = mol_ld(parent + p);
    if (gp == p) return p;
    mol_st(parent + cur, gp);   // cur is no root and never becomes one again; gp is one of its ancestors
    cur = gp;
    p = mol_ld(parent + cur);
  }
  return cur;
}

__device__ __forceinline__ void mol_unite(int* parent, int a, int b) {
  int ra = mol_find(parent, a), rb = mol_find(parent, b);
  while (ra != rb) {
    const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    // hi had been hooked by somebody else: old < hi is its parent now.  max(ra, rb) < hi from here on.
    ra = mol_find(parent, old);
    rb = mol_find(parent, lo);
  }
}

// sum of v over the wave added to *dst by one lane; every lane of the wave must call
__device__ __forceinline__ void mol_wave_add(unsigned long long* dst, unsigned long long v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}
__device__ __forceinline__ void mol_wave_max(unsigned long long* dst, unsigned long long v) {
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0 && v) atomicMax(dst, v);
}

__device__ __forceinline__ unsigned long long mol_hash(unsigned long long k) {   // splitmix64 finaliser
  k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27; k *= 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

__global__ __launch_bounds__(256) void mol_init_kernel(MolArgs a) {
  const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  for (long long t = t0; t < a.nlocal; t += stride) { a.parent[t] = (int)t; a.open_atom[t] = 0; a.open_root[t] = 0; }
  for (long long t = t0; t < (long long)a.nlocal * a.S; t += stride) a.comp[t] = 0;
  for (long long t = t0; t < a.table_size; t += stride) { a.keys[t] = kMolEmpty; a.cnt[t] = 0; }
  if (t0 < kMolCounters) a.counters[t0] = 0;
}

__global__ __launch_bounds__(256) void mol_union_kernel(MolArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long ii = t >> 4;
  const int sub = (int)(t & 15);
  unsigned long long nbond = 0;
  if (ii < a.nlocal) {
    const int i = a.ilist[ii];
    if ((unsigned)i < (unsigned)a.nlocal) {
      const int si = a.species[i];
      const double* cut_i = a.cut2 + (size_t)si * a.S;
      const double xi = a.x[3 * (size_t)i], yi = a.x[3 * (size_t)i + 1], zi = a.x[3 * (size_t)i + 2];
      const int* seg = a.jlist + a.nbr_off[ii];
      const int n = a.numneigh[ii];
      bool open = false;
      for (int k = sub; k < n; k += 16) {
        const int j = seg[k];
        if ((unsigned)j >= (unsigned)a.ntotal) continue;
        const double c2 = cut_i[a.species[j]];
        if (!(c2 > 0.0)) continue;   // never bonded: rejected before the position is loaded
        const double dx = a.x[3 * (size_t)j] - xi, dy = a.x[3 * (size_t)j + 1] - yi, dz = a.x[3 * (size_t)j + 2] - zi;
        if (!(dx * dx + dy * dy + dz * dz <= c2)) continue;
        nbond++;
        long long o = j;
        if (j >= a.nlocal) o = a.owner ? a.owner[j - a.nlocal] : -1;
        if (o < 0 || o >= a.nlocal) open = true;   // a foreign ghost: an atom of another rank
        else if ((int)o != i) mol_unite(a.parent, i, (int)o);
      }
      if (open) a.open_atom[i] = 1;
    }
  }
  mol_wave_add(a.counters + MOL_NBONDS, nbond);
}

__global__ __launch_bounds__(256) void mol_flatten_kernel(MolArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nlocal) return;
  const int r = mol_find(a.parent, (int)i);
  if (a.mol_of_atom) a.mol_of_atom[i] = r;
  atomicAdd(a.comp + (size_t)r * a.S + a.species[i], 1);
  if (a.open_atom[i]) a.open_root[r] = 1;   // every writer stores the same value
}

__global__ __launch_bounds__(256) void mol_tally_kernel(MolArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  unsigned long long is_mol = 0, is_open = 0, size = 0, open_atoms = 0;
  if (i < a.nlocal && a.parent[i] == (int)i) {
    const int* c = a.comp + (size_t)i * a.S;
    // the key: `bits` bits per species; a count at or above the field's largest value does not fit (the largest value itself
    // is left out so that no key equals the empty marker)
    const int bits = a.S > 2 ? 64 / a.S : 32;
    const unsigned long long fmax = (1ull << bits) - 1;
    unsigned long long key = 0;
    bool fits = true;
    for (int s = 0; s < a.S; s++) {
      const unsigned long long v = (unsigned long long)c[s];
      size += v;
      fits = fits && v < fmax;
      key |= (v & fmax) << (s * bits);
    }
    is_mol = 1;
    if (a.open_root[i]) {
      is_open = 1;
      open_atoms = size;
    } else if (fits) {
      unsigned slot = (unsigned)mol_hash(key) & (unsigned)(a.table_size - 1);
      for (int probe = 0; probe < a.table_size; probe++) {   // at most half the slots are ever taken
        const unsigned long long prev = atomicCAS(a.keys + slot, kMolEmpty, key);
        if (prev == kMolEmpty || prev == key) { atomicAdd(a.cnt + slot, 1); break; }
        slot = (slot + 1) & (unsigned)(a.table_size - 1);
      }
    } else {
      const unsigned long long k = atomicAdd(a.counters + MOL_NOVF, 1ull);
      if (k < (unsigned long long)a.ovf_cap) a.ovf[k] = (int)i;
    }
  }
  mol_wave_add(a.counters + MOL_NMOL, is_mol);
  mol_wave_add(a.counters + MOL_NOPEN, is_open);
  mol_wave_add(a.counters + MOL_OPEN_ATOMS, open_atoms);
  mol_wave_max(a.counters + MOL_LARGEST, size);
}

// threads [0, table_size): table slots; [table_size, table_size + ovf_cap): the molecules too large for a key
__global__ __launch_bounds__(256) void mol_decode_kernel(MolArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int W = a.S + 1;
  if (t < a.table_size) {
    const unsigned long long key = a.keys[t];
    if (key == kMolEmpty) return;
    const unsigned long long row = atomicAdd(a.counters + MOL_NDISTINCT, 1ull);
    if (!a.formula || row >= (unsigned long long)a.formula_cap) return;
    const int bits = a.S > 2 ? 64 / a.S : 32;
    const unsigned long long fmax = (1ull << bits) - 1;
    int* out = a.formula + (size_t)row * W;
    for (int s = 0; s < a.S; s++) out[s] = (int)((key >> (s * bits)) & fmax);
    out[a.S] = a.cnt[t];
    return;
  }
  const long long k = t - a.table_size;
  unsigned long long novf = a.counters[MOL_NOVF];
  if (novf > (unsigned long long)a.ovf_cap) novf = (unsigned long long)a.ovf_cap;
  if (k >= (long long)novf) return;
  // molecules of one composition make one row: the one with the smallest root writes it
  const int r = a.ovf[k];
  const int* c = a.comp + (size_t)r * a.S;
  int same = 0;
  for (unsigned long long m = 0; m < novf; m++) {
    const int q = a.ovf[m];
    const int* d = a.comp + (size_t)q * a.S;
    bool eq = true;
    for (int s = 0; s < a.S; s++) eq = eq && c[s] == d[s];
    if (!eq) continue;
    if (q < r) return;
    same++;
  }
  const unsigned long long row = atomicAdd(a.counters + MOL_NDISTINCT, 1ull);
  if (!a.formula || row >= (unsigned long long)a.formula_cap) return;
  int* out = a.formula + (size_t)row * W;
  for (int s = 0; s < a.S; s++) out[s] = c[s];
  out[a.S] = same;
}

__global__ void mol_summary_kernel(MolArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || !a.summary) return;
  a.summary[0] = (long long)a.counters[MOL_NMOL];
  a.summary[1] = (long long)a.counters[MOL_NDISTINCT];
  a.summary[2] = (long long)a.counters[MOL_NOPEN];
  a.summary[3] = (long long)a.counters[MOL_NBONDS];
  a.summary[4] = (long long)a.counters[MOL_LARGEST];
  a.summary[5] = (long long)a.counters[MOL_OPEN_ATOMS];
}

inline unsigned mol_blocks(long long threads) { return (unsigned)std::max<long long>((threads + 255) / 256, 1); }

}  // namespace

void launch_find_molecules(const MolArgs& a, hipStream_t st) {
  const long long init = std::max<long long>((long long)a.nlocal * a.S, a.table_size);
  hipLaunchKernelGGL(mol_init_kernel, dim3(std::min(mol_blocks(init), 4096u)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(mol_union_kernel, dim3(mol_blocks((long long)a.nlocal * 16)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(mol_flatten_kernel, dim3(mol_blocks(a.nlocal)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(mol_tally_kernel, dim3(mol_blocks(a.nlocal)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(mol_decode_kernel, dim3(mol_blocks((long long)a.table_size + a.ovf_cap)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(mol_summary_kernel, dim3(1), dim3(64), 0, st, a);
  note_launch_error(hipGetLastError());
}

}  // namespace ani
