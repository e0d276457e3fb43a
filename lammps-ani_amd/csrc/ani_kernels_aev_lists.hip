// ani_kernels_aev_lists.hip — the lists the AEV fast path starts from: the rebuild-time sort of every neighbour segment by
// species, the per-step compaction into the compact-list record (ani_aev_device.h), the fill of the stream tables; and which
// path a model takes (aev_fast_path, aev_compact_stride, stream_tab_supported).
#include "ani_aev_launch.h"
#include "ani_aev_stream.h"

namespace ani {

// =====================================================================================================
// rebuild time: stable sort of every centre's neighbour segment by neighbour species
// =====================================================================================================
__global__ __launch_bounds__(256) void sort_jlist_kernel(const int* __restrict__ species, const int* __restrict__ nbr_off,
                                                         const int* __restrict__ numneigh, const int* __restrict__ jin,
                                                         int* __restrict__ jout, int nlocal, int S, int present, int in_stride) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ii = blockIdx.x * 4 + wave;
  if (ii >= nlocal) return;
  const int beg = nbr_off[ii], n = numneigh[ii];
  // the unsorted entries: dense segments like the output, or rows of a fixed capacity (the one-pass list build)
  jin += in_stride ? (long long)ii * in_stride - beg : 0LL;
  int outpos = 0;
  for (int s = 0; s < S; s++) {
    if (!((present >> s) & 1)) continue;   // a species that occurs nowhere in the system: no pass over the list for it
    for (int base = 0; base < n; base += 64) {
      const int q = base + lane;
      const int j = q < n ? jin[beg + q] : 0;
      const bool hit = q < n && species[j] == s;
      const unsigned long long m = __ballot(hit);
      if (hit) jout[beg + outpos + lanes_below(m)] = j;
      outpos += __popcll(m);
    }
  }
}

void launch_sort_jlist(const int* d_species, const int* d_nbr_off, const int* d_numneigh, const int* d_jin, int* d_jout,
                       int nlocal, int S, int present_mask, hipStream_t st, int in_stride) {
  if (nlocal <= 0) return;
  hipLaunchKernelGGL(sort_jlist_kernel, dim3((nlocal + 3) / 4), dim3(256), 0, st, d_species, d_nbr_off, d_numneigh, d_jin, d_jout,
                     nlocal, S, present_mask, in_stride);
}

// ---- per-step compaction: nbr_compact_kernel (the record it writes: ani_aev_device.h) ----
// Persistent waves, software-pipelined across rows: wave w walks rows w, w + W, ...; while row c is screened, the
// position gathers of c+1, the list loads of c+2 and the row_info of c+3 are in flight.  NCH 64-entry chunks of a list
// are held per stage; longer lists take further super-chunks loaded in place.
// vmcnt counts loads and stores together, in order: a wait for prefetched data that is placed AFTER a row's stores
// waits for those stores as well (a full write round trip per row).  So every value a later row needs is waited for
// (touch()) before the current row's stores are issued, and the stores come last in the iteration; row_info is loaded
// through an index the compiler cannot prove uniform, or it would load + v_readfirstlane it on the spot (draining
// every gather in flight) -- it is made scalar only when its row is started.
constexpr int kWavesC = 4;
template <int NCH>
__global__ __launch_bounds__(64 * kWavesC, NCH >= 4 ? 4 : 5) void nbr_compact_kernel(AevParams p, AevArgs a, int cap) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int nw = gridDim.x * kWavesC;
  int k = blockIdx.x * kWavesC + wave;
  if (k >= a.kcount) return;
  const int cap2 = a.cl_stride - kMaxAng;   // room of the radial-only stream
  int4 info = load_info(a, k), info1 = load_info(a, k + nw), info2 = load_info(a, k + 2 * nw);
  int jj[NCH], jj1[NCH];
  float4 xi, xx[NCH];
  load_j(a, info, lane, jj);
  load_j(a, info1, lane, jj1);
  gather_x(a, info, jj, xi, xx);
  while (k < a.kcount) {
    // next stages
    float4 xi1, xx1[NCH];
    gather_x(a, info1, jj1, xi1, xx1);
    int jj2[NCH];
    load_j(a, info2, lane, jj2);
    const int4 info3 = load_info(a, k + 3 * nw);

    const int4 inf = uniform4(info);
    const int row = inf.w;
    int4* hdr = a.cl_hdr + 2 * (size_t)row;
    const int i = inf.x, beg = inf.y, n = inf.x < 0 ? 0 : inf.z;
    float4* oxyz = a.cl_xyz + (size_t)row * a.cl_stride;
    int* oj = a.cl_j + (size_t)row * a.cl_stride;
    int nA = 0, nR = 0;    // wave-uniform stream lengths
    int ca = 0, c2 = 0;    // lane s: entries of species s in either stream
    float4 dd[NCH];
    int pos[NCH];          // output slot of this lane's candidate of chunk c, -1: screened out
    auto screen = [&](int c, bool valid, const float4& xj, float4& d, int& sp) -> int {
      d.x = xj.x - xi.x; d.y = xj.y - xi.y; d.z = xj.z - xi.z;
      d.w = __builtin_amdgcn_sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
      sp = __float_as_int(xj.w);
      const bool in_a = valid && d.w <= p.Rca;
      const bool in_2 = valid && !in_a && (p.compat || d.w <= p.Rcr);
      const unsigned long long mA = __ballot(in_a), m2 = __ballot(in_2);
      const int pA = nA + lanes_below(mA), p2 = nR + lanes_below(m2);
      for (int s = 0; s < p.S; s++) {
        const int k1 = __popcll(__ballot(in_a && sp == s)), k2 = __popcll(__ballot(in_2 && sp == s));
        if (lane == s) { ca += k1; c2 += k2; }
      }
      nA += __popcll(mA);
      nR += __popcll(m2);
      return (in_a && pA < kMaxAng) ? pA : ((in_2 && p2 < cap2) ? kMaxAng + p2 : -1);
    };
    int spv[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      pos[c] = -1;
      spv[c] = 0;
      dd[c] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (64 * c < n) pos[c] = screen(c, 64 * c + lane < n, xx[c], dd[c], spv[c]);   // wave-uniform test
    }
    // everything the later rows need has now to be in registers: the stores below must not be waited for
    touch(xi1); touch(info3);
#pragma unroll
    for (int c = 0; c < NCH; c++) { touch(xx1[c]); touch(jj2[c]); }
#pragma unroll
    for (int c = 0; c < NCH; c++)
      if (pos[c] >= 0) { oxyz[pos[c]] = dd[c]; oj[pos[c]] = cl_pack(jj[c], spv[c]); }
    for (int base0 = 64 * NCH; base0 < n; base0 += 64) {   // more than 64 * NCH list entries: rare, loaded in place
      const int q = base0 + lane;
      const int j = q < n ? a.jlist[beg + q] : i;
      const float4 xj = a.xyzs[j];
      float4 d;
      int sp;
      const int ps = screen(0, q < n, xj, d, sp);
      if (ps >= 0) { oxyz[ps] = d; oj[ps] = cl_pack(j, sp); }
    }
    // capacity of the consumers' LDS lists: never a silent truncation -- the row is skipped and the error flag raised
    const bool over = nA > kMaxAng || nR > cap2 || nA + nR > cap;
    if (lane < 8) {
      reinterpret_cast<unsigned char*>(hdr)[8 + lane] = (unsigned char)ca;
      reinterpret_cast<unsigned short*>(hdr)[8 + lane] = (unsigned short)c2;
    }
    if (lane == 0) {
      reinterpret_cast<int*>(hdr)[0] = (over || inf.x < 0) ? -1 : i;
      reinterpret_cast<int*>(hdr)[1] = (nA + nR) | (nA << 16) | (__float_as_int(xi.w) << 24);
      if (over) atomicOr(a.err_flag, 1);
    }
    info = info1; info1 = info2; info2 = info3;
    xi = xi1;
#pragma unroll
    for (int c = 0; c < NCH; c++) { jj[c] = jj1[c]; xx[c] = xx1[c]; jj1[c] = jj2[c]; }
    k += nw;
  }
}

// Fills one tuple's run of a table with what the arithmetic decode yields: one wave per tuple, the counts of the tuple as the
// group starts of an LDS slice that holds nothing else.
template <int NA, int NZ, bool BWD>
__global__ __launch_bounds__(64) void stream_table_kernel(AevParams p, int nt, int4* desc, unsigned* words, int fill) {
  __shared__ int s_astart[24];
  __shared__ int s_tb[kMaxBuckets * 8];
  constexpr int STEP = BWD ? 32 : 64;
  const int lane = threadIdx.x, t = blockIdx.x;
  FastLds L{};
  L.astart = s_astart;
  L.tb = s_tb;
  const int n0 = p.S == 1 ? t : t / (nt + 1), n1 = p.S == 1 ? 0 : t % (nt + 1);
  if (lane <= p.S) s_astart[lane] = lane == 0 ? 0 : (lane == 1 ? n0 : n0 + n1);
  wave_sync();
  int nbk;
  const int total = BWD ? build_pair_table<NA, NZ>(p, lane, L, nbk) : build_bucket_table<NA, NZ>(p, lane, L, nbk);
  wave_sync();
  const int reserved = (total + STEP - 1) / STEP * STEP;
  if (!fill) {
    if (lane == 0) desc[t] = make_int4(0, total, nbk, reserved);
    return;
  }
  unsigned* out = words + desc[t].x;
  for (int v = lane; v < reserved; v += 64) {
    unsigned w;
    if constexpr (BWD) {
      int ia0, ib0, off0, pos0, ia1, ib1, off1, pos1;
      bool v0, v1;
      stream_pair_half(L, nbk, v, 0, ia0, ib0, off0, pos0, v0);
      stream_pair_half(L, nbk, v, 1, ia1, ib1, off1, pos1, v1);
      int e = 0;
      for (int k = 1; k < nbk; k++)
        if (v >= L.tb[8 * k]) e = k;
      const int tri = L.tb[8 * e + 6], bk = (off0 - p.radial_len) / (NA * NZ);
      w = (unsigned)ia0 | ((unsigned)ib0 << 8) | ((unsigned)pos0 << 16) | ((unsigned)bk << 24) | ((unsigned)(tri ? 1 : 0) << 29) |
          ((unsigned)(v0 ? 1 : 0) << 30) | ((unsigned)(v1 ? 1 : 0) << 31);
    } else {
      int ia, ib, off;
      bool valid;
      stream_pair(L, nbk, v, ia, ib, off, valid);
      const int bk = (off - p.radial_len) / (NA * NZ);
      w = (unsigned)ia | ((unsigned)ib << 8) | ((unsigned)bk << 16) | ((unsigned)(valid ? 1 : 0) << 24);
    }
    out[v] = w;
  }
}

bool aev_fast_path(const AevParams& p, int max_numneigh) { return fast_plan(p, max_numneigh).fast(); }

int aev_compact_stride(const AevParams& p, int max_numneigh) {
  const FastPlan pl = fast_plan(p, max_numneigh);
  return pl.fast() ? kMaxAng + pl.cap : 0;
}

void launch_nbr_compact(const AevParams& p, const AevArgs& a, int max_numneigh, hipStream_t st) {
  const FastPlan pl = fast_plan(p, max_numneigh);
  if (a.kcount <= 0 || !pl.fast()) return;
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(persistent_blocks(kernel, a.kcount, kWavesC, 0)), dim3(64 * kWavesC), 0, st, p, a, pl.cap);
  };
  dispatch([&](auto NCH) { go(nbr_compact_kernel<NCH>); }, one_of<2, 3, 4>{pl.chunks});
}

// the tables hold what the fast kernels would decode: whatever the list lengths, so the plan of an empty list says it
static int stream_tab_kind(const AevParams& p) { return (p.S == 1 || p.S == 2) ? fast_plan(p, 0).kind : 0; }
bool stream_tab_supported(const AevParams& p) { return stream_tab_kind(p) != 0; }

void launch_stream_table(const AevParams& p, int nt, bool backward, int4* d_desc, unsigned* d_words, int fill, hipStream_t st) {
  const int n = stream_tab_tuples(p.S, nt);
  if (n <= 0) return;
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(n), dim3(64), 0, st, p, nt, d_desc, d_words, fill); };
  dispatch([&](auto K, auto BWD) { go(stream_table_kernel<kGridNA<K>, kGridNZ<K>, BWD != 0>); }, one_of<1, 2>{stream_tab_kind(p)},
           one_of<0, 1>{backward});
}

}  // namespace ani
