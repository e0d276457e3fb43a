// ani_aev_device.h — device code that the AEV translation units share (ani_kernels_aev_{lists,fast,generic}.hip): wave
// primitives, the LDS layout of the fast path, the compact-list record with its loads, the stamp macros of the measurement
// build.  The pair streams and the row tickets are in ani_aev_stream.h, the host side of a launch in ani_aev_launch.h.
//
// AEV (radial + angular symmetry functions) forward and analytic backward over the
// LAMMPS full neighbour list.  Replaces torchani's cuaev / pyaev (not in the reference tree; call sites
// models/lammps_ani.py:277-296) and the autograd pass through it (models/lammps_ani.py:197-206).
//
// One wavefront (64 lanes) per centre atom, four centres per workgroup, no workgroup barriers: each wave owns a
// private slice of LDS.  At rebuild time every centre's neighbour segment is sorted by neighbour species
// (sort_jlist_kernel), so the screened lists built per step come out grouped by species and every
// (species) / (species pair) block of the AEV row has exactly one contiguous group of contributors.
//
// Fast path (NR = 16 radial shifts, NA x NZ = 8x4 (ANI-2x) or 4x8 (ANI-1x) angular grid, <= 8 species):
//   compaction : coalesced jlist loads, float4 position gathers, ballot/popcount compaction into LDS.
//   radial     : per species group, lanes = (4 neighbour slots) x (16 shifts); 2 xor-shuffles; plain store.
//   angular    : the pairs of all non-empty species-pair buckets form ONE padded stream (bucket starts are
//                multiples of Q = 64/NA).  Per chunk of 64 pairs: phase 1, lane = pair, computes the NA radial
//                and NZ angular factors once and parks them in LDS; phase 2, lane = (slot q, shift a), walks
//                the chunk in NA steps with NZ register accumulators that are flushed (log2(Q) xor-shuffles,
//                plain 16-byte stores) whenever the bucket changes.  No LDS atomics, bitwise reproducible.
//   backward   : same stream; lane = pair contracts the 32 dE/dAEV entries of its bucket against the factor
//                derivatives and adds the two gradient vectors to per-neighbour LDS accumulators; one global
//                float atomic per neighbour component scatters the force; the virial is reduced per wave.
// Generic path (any NR/NA/NZ/S): the first-generation kernels with LDS float atomics, kept for odd model
// shapes (e.g. the unit-test "tiny" model).
//
// Transcendentals on the fast path are the hardware ones (v_exp_f32, v_log_f32, v_cos_f32, v_sin_f32, v_rcp_f32,
// v_rsq_f32), as the reference's cuaev is built with -use_fast_math (src/ani_csrc/CMakeLists.txt:12-20).
// Formulas and their derivatives are the ones restated in oracle/ani_oracle.c.
#pragma once
#include "ani_kernels.h"

namespace ani {

constexpr int kWaves = 4;    // centres per workgroup: forward fast path and generic kernels
constexpr int kWavesB = 4;   // backward fast path
// waves per SIMD the fast kernels are compiled for (the second __launch_bounds__ argument).  Forcing more was measured and
// not taken (profiles/r03_ablation_notes.md): backward 5 -> 0.294 against 0.297 ms (noise), 6 -> spills; forward 7 -> 0.209
// against 0.207 ms.
constexpr int kBwdMinWaves = 4;
constexpr int kFwdMinWaves = 4;
constexpr int kFusedMinWaves = 4;
constexpr int kAevMax = 1024;   // LDS floats reserved for one AEV row (ANI-2x: 1008)
constexpr int kMaxBuckets = 36; // species pairs on the fast path (S <= 8)

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
}
// inclusive prefix sum over the 64 lanes without LDS: four DPP shifts inside each row of 16 lanes, then the row totals
// passed on with row_bcast:15 (rows 1, 3) and row_bcast:31 (rows 2, 3)
__device__ __forceinline__ int wave_incl_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return v;
}
__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float flog2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float frsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float fcos_rev(float rev) { return __builtin_amdgcn_cosf(rev); }  // cos(2 pi rev)
__device__ __forceinline__ float fsin_rev(float rev) { return __builtin_amdgcn_sinf(rev); }
constexpr float kLog2e = 1.4426950408889634f;

// v + v[lane ^ OFF] without an LDS round trip: OFF = 1, 2, 4, 8 as DPP moves inside a row of 16 lanes, OFF = 16 / 32
// with the gfx950 row / half-wave swaps (both operands the same register: one result holds the even rows or the lower
// half everywhere, the other the odd rows or the upper half)
template <int OFF>
__device__ __forceinline__ float xor_sum(float v) {
  const int x = __float_as_int(v);
  if constexpr (OFF == 1) {
    return v + __int_as_float(__builtin_amdgcn_mov_dpp(x, 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
  } else if constexpr (OFF == 2) {
    return v + __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
  } else if constexpr (OFF == 4) {
    int y = __builtin_amdgcn_update_dpp(x, x, 0x104, 0xf, 0x5, false);  // row_shl:4 into banks 0,2
    y = __builtin_amdgcn_update_dpp(y, x, 0x114, 0xf, 0xa, false);      // row_shr:4 into banks 1,3
    return v + __int_as_float(y);
  } else if constexpr (OFF == 8) {
    return v + __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x128, 0xf, 0xf, true));  // row_ror:8
  } else if constexpr (OFF == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
  } else {
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
}

// diagnostic build (-DABLB_STAMPS): wave 0 of every backward workgroup adds the shader-clock cycles it spent in each phase
// of a centre to g_bwd_stamps (read through ani_debug_fused_stamps); no stamp executes in the shipped kernel
#ifdef ABLB_STAMPS
#define BWD_STAMP(k)                                                                          \
  do {                                                                                        \
    unsigned long long _t;                                                                    \
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory"); \
    stamp_acc[k] += _t - stamp_prev;                                                          \
    stamp_prev = _t;                                                                          \
  } while (0)
#define BWD_STAMP_VM(k)                                                                       \
  do {                                                                                        \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                          \
    BWD_STAMP(k);                                                                             \
  } while (0)
#define BWD_STAMP_PARAMS , unsigned long long& stamp_prev, unsigned long long (&stamp_acc)[8]
#define BWD_STAMP_ARGS , stamp_prev, stamp_acc
#else
#define BWD_STAMP(k) do {} while (0)
#define BWD_STAMP_VM(k) do {} while (0)
#define BWD_STAMP_PARAMS
#define BWD_STAMP_ARGS
#endif

// unordered pair index t -> (a, b), a < b < n, row-major over the strict upper triangle
__device__ __forceinline__ void decode_pair(int t, int n, int& a, int& b) {
  // closed form + one branch-free correction step each way; all quantities < 2^14, so 24-bit multiplies are exact
  const float fn = (float)(2 * n - 1);
  int aa = (int)((fn - __builtin_amdgcn_sqrtf(fn * fn - 8.f * (float)t)) * 0.5f);
  aa = max(0, min(aa, n - 2));
  const int n2 = 2 * n - 1;
  int s0 = __mul24(aa, n2 - aa) >> 1;              // first pair index of row aa
  const bool dn = s0 > t;
  aa -= dn ? 1 : 0;
  s0 = dn ? (__mul24(aa, n2 - aa) >> 1) : s0;
  const int s1 = __mul24(aa + 1, n2 - aa - 1) >> 1;  // first pair index of row aa + 1
  const bool up = s1 <= t;
  aa += up ? 1 : 0;
  s0 = up ? s1 : s0;
  a = aa;
  b = aa + 1 + (t - s0);
}
__device__ __forceinline__ int triu_index(int s1, int s2, int S) {
  const int lo = s1 < s2 ? s1 : s2, hi = s1 < s2 ? s2 : s1;
  return lo * S - lo * (lo - 1) / 2 + (hi - lo);
}

// =====================================================================================================
// fast path
// =====================================================================================================
// The backward kernel's per-neighbour gradient accumulators in LDS take several adds per pair.  On gfx950 an LDS fp32 add
// (ds_add_f32, also ds_pk_add_f16) is executed ONE LANE AT A TIME, ~3 cycles per active lane -- 192 cycles for a full wave,
// the CU's LDS blocked meanwhile -- whereas ds_add_f64 takes 8 cycles per wave-instruction, like the integer adds
// (tools/lds_rmw_probe.hip, profiles/r03_lds_rmw_probe.log).  So the accumulators are doubles: one v_cvt_f64_f32 per
// value added, 6 instead of 3 words per neighbour, and sums that are more accurate on top.
constexpr int kGdWords = 6;   // LDS words per angular neighbour: three doubles

struct FastLds {
  // carved from dynamic LDS, per wave
  float4* ad;     // [kMaxAng] angular neighbours dx,dy,dz,r
  float* afc;     // [kMaxAng] fc(r; Rca)
  float* row;     // [rowf] forward: AEV row; backward: dE/dAEV row
  float* pf2;     // [64*NA] forward
  float* pf1;     // [64*NZ] forward
  int* tb;        // [kMaxBuckets*8] bucket table
  int* rstart;    // [kMaxSpecies+1]
  int* astart;    // [kMaxSpecies+1]
  float* rr;      // [cap] forward: radial list r
  float* rfc;     // [cap] forward: fc(r; Rcr)
  int* aj;        // [kMaxAng] backward: atom index of the angular neighbours
  double* gd;     // [3*kMaxAng] backward: dE/d(displacement) of the angular neighbours (fp64: see above)
  float* gt;      // [3*64] backward: staging of one chunk of radial-only gradients for the force scatter
  int* jt;        // [64]   ... and of their atom indices
};

__host__ __device__ constexpr int fast_wave_floats(int cap, bool bwd) {
  // both: ad 4*kMaxAng + row kAevMax + tb kMaxBuckets*8 + starts 2*24
  // forward adds afc, the phase-1 factor buffers pf (64*12) and r, fc per radial neighbour;
  // backward adds afc, aj and gd[3] (fp64) per ANGULAR neighbour and the 4*64 staging words (the radial-only neighbours never
  // touch LDS)
  return 4 * kMaxAng + kAevMax + kMaxBuckets * 8 + 48 + (bwd ? (2 + kGdWords) * kMaxAng + 256 : kMaxAng + 64 * 12 + 2 * cap);
}
// same with the AEV row sized for the columns actually in use (rowf floats, multiple of 64)
// ... and the bucket table for the species pairs of the model in use (S (S + 1) / 2 entries of 8 words: 3 for pruned water, 28 for
// seven species): the 264 words a water run does not need are the difference between five and six forward workgroups per CU
__host__ __device__ constexpr int table_words(int S) { return 8 * (S * (S + 1) / 2); }
__host__ __device__ constexpr int fast_wave_floats_row(int cap, bool bwd, int rowf, int S) {
  return fast_wave_floats(cap, bwd) - kAevMax + rowf - kMaxBuckets * 8 + table_words(S);
}

template <int NA, int NZ>
__device__ __forceinline__ FastLds carve(float* base, int cap, bool bwd, int rowf) {
  FastLds L{};
  float* p = base;
  // fixed-size pieces first so that their offsets from the wave base are compile-time immediates
  L.ad = reinterpret_cast<float4*>(p); p += 4 * kMaxAng;
  L.rstart = reinterpret_cast<int*>(p); p += 24;
  L.astart = reinterpret_cast<int*>(p); p += 24;
  if (!bwd) {
    L.afc = p; p += kMaxAng;
    L.pf2 = p; p += 64 * NA;
    L.pf1 = p; p += 64 * NZ;
    L.row = p; p += rowf;
    L.rr = p; p += cap;
    L.rfc = p; p += cap;
    L.tb = reinterpret_cast<int*>(p);   // sized by the model's species count (table_words): last
  } else {
    L.aj = reinterpret_cast<int*>(p); p += kMaxAng;
    L.gd = reinterpret_cast<double*>(p); p += kGdWords * kMaxAng;   // 8-byte aligned: every piece in front of it is an even number of words
    L.afc = p; p += kMaxAng;
    L.gt = p; p += 3 * 64;
    L.jt = reinterpret_cast<int*>(p); p += 64;
    L.row = p; p += rowf;
    L.tb = reinterpret_cast<int*>(p);
  }
  return L;
}

// LDS words per wave of the backward kernel: the armed instantiation (AV) stages the radial-only displacements behind the slice
__host__ __device__ constexpr int bwd_wave_floats(int cap, int rowf, int S, bool av) {
  return fast_wave_floats_row(cap, true, rowf, S) + (av ? 3 * 64 : 0);
}
static_assert((fast_wave_floats(0, true) + 3 * 64) * 4 * kWavesB <= 160 * 1024, "armed backward LDS");

// ---- per-step compaction (its own kernel) -------------------------------------------------------------------
// nbr_compact_kernel screens the (species-sorted) candidate list of every centre ONCE per step and leaves, per AEV row,
//   cl_hdr[2*row + 0] = {centre atom i (-1: padding row / skipped), nrad | nang << 16 | centre species << 24,
//                        angular neighbours of species 0..3 (u8 each), of species 4..7}
//   cl_hdr[2*row + 1] = radial-only neighbours (Rca < r <= Rcr) per species, 8 x u16
//   cl_xyz[row*stride + t]            , t < nang : {dx, dy, dz, r} of the neighbours inside Rca, in list (= species) order
//   cl_xyz[row*stride + kMaxAng + u]  , u < nrad - nang : the same for the radial-only neighbours
//   cl_j  [...]                       their atom indices (backward pass: force scatter)
// Two append-only streams per row, so the kernel is ONE pass over the candidates with two ballots per 64 of them.
// The forward and the backward kernel both start from these lists (coalesced 16-byte loads addressed by row: one
// centre ahead is all the prefetch they need) instead of each walking the ~150 candidates again: the walk is a chain of
// dependent loads (list -> positions) with little arithmetic, exactly what a small kernel at eight waves per SIMD
// hides and a 100-170 VGPR compute kernel at three or four does not.
// a compact-list entry of cl_j: the neighbour's atom index with its (compact) species in the top four bits, so that the backward
// kernel's radial stage knows a neighbour's dE/dAEV row without walking the per-species counts (27 scalars that spilled)
constexpr int kClIndexBits = 28;
__device__ __forceinline__ int cl_pack(int j, int sp) { return j | (sp << kClIndexBits); }
__device__ __forceinline__ int cl_index(int e) { return e & ((1 << kClIndexBits) - 1); }
__device__ __forceinline__ int cl_species(int e) { return (unsigned)e >> kClIndexBits; }
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ void touch(int v) { asm volatile("" ::"v"(v)); }
__device__ __forceinline__ void touch(float v) { asm volatile("" ::"v"(v)); }
__device__ __forceinline__ void touch(const float4& v) { asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w)); }
__device__ __forceinline__ void touch(const int4& v) { asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w)); }
__device__ __forceinline__ int4 uniform4(const int4& v) {
  return make_int4(__builtin_amdgcn_readfirstlane(v.x), __builtin_amdgcn_readfirstlane(v.y), __builtin_amdgcn_readfirstlane(v.z),
                   __builtin_amdgcn_readfirstlane(v.w));
}
// The fast kernels walk the k-th row of a range, k in [0, a.kcount): row = a.row_list[a.k0 + k], or a.k0 + k without a
// list (every row: k0 = 0, kcount = nrows).  Lists: the rows with / without a ghost atom among their candidates, so
// that a step can be cut where the ghost exchange has to happen (ani_step_* in ani_hip.h).
__device__ __forceinline__ int4 load_info(const AevArgs& a, int k) {   // per-lane copy; k past the end reads the last row
  const int kk = opaque(k < a.kcount ? k : a.kcount - 1);
  const int r = a.row_list ? a.row_list[a.k0 + kk] : a.k0 + kk;
  int4 info = a.row_info[r];
  info.w = r;   // the row travels with its stage (the centre's position in ilist, which sat here, is not used below)
  return info;
}
template <int NCH>
__device__ __forceinline__ void load_j(const AevArgs& a, const int4 info, int lane, int (&jj)[NCH]) {
  const int i = info.x < 0 ? 0 : info.x;
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    const int q = 64 * c + lane;
    jj[c] = q < info.z ? a.jlist[info.y + q] : i;
  }
}
template <int NCH>
__device__ __forceinline__ void gather_x(const AevArgs& a, const int4 info, const int (&jj)[NCH], float4& xi, float4 (&xx)[NCH]) {
  xi = a.xyzs[info.x < 0 ? 0 : info.x];
#pragma unroll
  for (int c = 0; c < NCH; c++) xx[c] = a.xyzs[jj[c]];
}

// What the forward / backward kernels load for a centre: first the header (wave-uniform, two 16-byte words), then the
// first NCH 64-entry chunks of its compact list in slot order -- slots [0, nang) are the angular region, slots
// [nang, nrad) the radial-only one -- so that a typical centre (nrad < 64) is ONE chunk with every lane busy instead
// of an angular chunk (a quarter of the lanes) and a radial-only chunk; for the backward pass also the atom indices and
// the dE/dAEV row.  No prefetch across centres (see ANI_PERSISTENT_LOOP).
typedef int hdr_t __attribute__((ext_vector_type(8)));
template <int NCH, bool BWD, int GR>
struct Loaded {
  float4 xx[NCH];
  int jj[BWD ? NCH : 1];
  float4 grow[BWD ? GR : 1];
};
__device__ __forceinline__ hdr_t load_header(const AevArgs& a, int row) {   // row is wave-uniform
  const int4* hp = a.cl_hdr + 2 * (size_t)row;
  const int4 h0 = hp[0], h1 = hp[1];
  hdr_t h;
  h[0] = __builtin_amdgcn_readfirstlane(h0.x); h[1] = __builtin_amdgcn_readfirstlane(h0.y);
  h[2] = __builtin_amdgcn_readfirstlane(h0.z); h[3] = __builtin_amdgcn_readfirstlane(h0.w);
  h[4] = __builtin_amdgcn_readfirstlane(h1.x); h[5] = __builtin_amdgcn_readfirstlane(h1.y);
  h[6] = __builtin_amdgcn_readfirstlane(h1.z); h[7] = __builtin_amdgcn_readfirstlane(h1.w);
  return h;
}
// The same through the scalar cache: the header is wave-uniform, a scalar load leaves eight vector moves out -- and it is counted
// by lgkmcnt, not by the in-order vmcnt queue, so it does not wait for the force atomics the wave still has in flight.
__device__ __forceinline__ hdr_t load_header_scalar(const AevArgs& a, int row) {   // row is wave-uniform
  const int4* hp = a.cl_hdr + 2 * (size_t)row;
  hdr_t h;
  asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(h) : "s"(hp) : "memory");
  return h;
}
// compact-list slot t (angular entries first, then the radial-only ones) -> index in the row's cl_xyz / cl_j
__device__ __forceinline__ int slot_index(int t, int nang) { return t < nang ? t : kMaxAng + (t - nang); }
template <int NCH, bool BWD, int GR>
__device__ __forceinline__ void load_lists(const AevParams& p, const AevArgs& a, int row, int nrad, int nang, int lane,
                                           Loaded<NCH, BWD, GR>& ld) {
  const float4* px = a.cl_xyz + (size_t)row * a.cl_stride;
  const int* pj = a.cl_j + (size_t)row * a.cl_stride;
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    const int t = 64 * c + lane;
    ld.xx[c] = t < nrad ? px[slot_index(t, nang)] : make_float4(0.f, 0.f, 0.f, 1.f);
    if constexpr (BWD) ld.jj[c] = t < nrad ? pj[slot_index(t, nang)] : 0;
  }
  if constexpr (BWD) {
    const int n4 = p.aev_stride >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(a.gaev + (size_t)row * p.aev_stride);
#pragma unroll
    for (int c = 0; c < GR; c++) ld.grow[c] = lane + 64 * c < n4 ? g4[lane + 64 * c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
__device__ __forceinline__ int hdr_nrad(const hdr_t& h) { return h[0] < 0 ? 0 : (h[1] & 0xffff); }
__device__ __forceinline__ int hdr_nang(const hdr_t& h) { return h[0] < 0 ? 0 : ((h[1] >> 16) & 0xff); }
__device__ __forceinline__ int hdr_species(const hdr_t& h) { return (h[1] >> 24) & 0xf; }

// scalar bookkeeping of a centre's compact list: starts of species k in the angular stream (as), in the radial-only
// stream (r2) and in the species-grouped radial order (rs); entry 8 holds the totals
struct Groups { int as[9], r2[9], rs[9]; };
__device__ __forceinline__ Groups unpack_groups(const hdr_t& h) {
  Groups g;
  g.as[0] = g.r2[0] = g.rs[0] = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int cak = (h[2 + (k >> 2)] >> (8 * (k & 3))) & 0xff, c2k = (h[4 + (k >> 1)] >> (16 * (k & 1))) & 0xffff;
    g.as[k + 1] = g.as[k] + cak;
    g.r2[k + 1] = g.r2[k] + c2k;
    g.rs[k + 1] = g.rs[k] + cak + c2k;
  }
  return g;
}
__device__ __forceinline__ void store_starts(const AevParams& p, const Groups& g, int nrad, int nang, int lane, FastLds& L) {
  int vr = nrad, va = nang;   // entries S.. of the start tables hold the totals
#pragma unroll
  for (int k = 7; k >= 0; k--)
    if (lane == k && k < p.S) { vr = g.rs[k]; va = g.as[k]; }
  if (lane <= p.S) { L.rstart[lane] = vr; L.astart[lane] = va; }
}

}  // namespace ani
