// ani_aev_fwd.h — forward pass of the AEV fast path: aev_forward_fast from the compact lists, aev_forward_fused with the
// per-step compaction inside (the design: head of ani_aev_device.h).  Kernel templates; ani_kernels_aev_fast.hip instantiates them.
#pragma once
#include "ani_aev_stream.h"

namespace ani {

// Forward: fill the wave's LDS lists from the prefetched compact list: the radial list {r, fc} grouped by species (inside
// a group the angular neighbours first), the angular list (the angular region as it stands, already in species order),
// group starts in L.rstart / L.astart.  All per-species bookkeeping is scalar.
template <int NCH>
__device__ __forceinline__ void unpack_lists(const AevParams& p, const AevArgs& a, int row, const hdr_t& h,
                                             const Loaded<NCH, false, 1>& ld, int lane, FastLds& L, int& nrad, int& nang) {
  nrad = hdr_nrad(h);
  nang = hdr_nang(h);
  const Groups g = unpack_groups(h);
  store_starts(p, g, nrad, nang, lane, L);
  const float half_inv_Rcr = 0.5f * p.pi_over_Rcr * 0.3183098861837907f;  // r/(2 Rcr) revolutions
  const float half_inv_Rca = 0.5f * p.pi_over_Rca * 0.3183098861837907f;
  const float4* __restrict__ px = a.cl_xyz + (size_t)row * a.cl_stride;
  for (int base = 0; base < nrad; base += 64) {
    const int c = base >> 6, t = base + lane;
    float4 v = make_float4(0.f, 0.f, 0.f, 1.f);
    if (c < NCH) {
#pragma unroll
      for (int k = 0; k < NCH; k++)
        if (c == k) v = ld.xx[k];
    } else if (t < nrad) {   // lists longer than the chunks held in registers: loaded in place
      v = px[slot_index(t, nang)];
    }
    if (t < nrad) {
      // w-th entry of the angular (ang) or the radial-only stream -> position in the LDS radial list
      const bool ang = t < nang;
      const int w = ang ? t : t - nang;
      int pos = w;   // species 0: the radial-only entries follow its as[1] angular ones
      int lead = g.as[1];
#pragma unroll
      for (int k = 1; k < 8; k++)
        if (k < p.S) {
          const int st = ang ? g.as[k] : g.r2[k];
          if (w >= st) { pos = g.rs[k] + (w - st); lead = g.as[k + 1] - g.as[k]; }
        }
      if (!ang) pos += lead;
      L.rr[pos] = v.w;
      L.rfc[pos] = 0.5f * fcos_rev(v.w * half_inv_Rcr) + 0.5f;
      if (ang) {
        L.ad[w] = v;
        L.afc[w] = 0.5f * fcos_rev(v.w * half_inv_Rca) + 0.5f;
      }
    }
  }
}

// forward_compute: the AEV row of one centre from the wave's LDS lists (radial list grouped by species, angular list, group
// starts) -- filled from the compact list by forward_centre, or straight from the candidate list by the fused kernel
// TAB: the centre may come with its place in the forward stream table (sc.on); without it, and in the instantiations without tables,
// the slots are decoded arithmetically
template <int NA, int NZ, bool TAB>
__device__ __forceinline__ void forward_compute(const AevParams& p, const AevArgs& a, FastLds& L, int row, int lane,
                                                StreamCur sc BWD_STAMP_PARAMS);

template <int NA, int NZ, int NCH, bool TAB>
__device__ __forceinline__ void forward_centre(const AevParams& p, const AevArgs& a, FastLds& L, int row, const hdr_t& h,
                                               const Loaded<NCH, false, 1>& pf, int lane, const StreamTab& tab BWD_STAMP_PARAMS) {
  StreamCur sc;
  if constexpr (TAB)   // the header's count bytes -> tuple -> descriptor and first word, in flight during the unpack and the radial stage
    sc = stream_begin<64>(tab.desc_f, tab.words_f, stream_tuple(p, tab, h[2] & 0xff, (h[2] >> 8) & 0xff), lane);
  for (int e = lane; e < (p.aev_stride >> 2); e += 64) reinterpret_cast<float4*>(L.row)[e] = make_float4(0, 0, 0, 0);
  int nrad, nang;
  unpack_lists<NCH>(p, a, row, h, pf, lane, L, nrad, nang);
  wave_sync();
  BWD_STAMP(2);   // unpack
  forward_compute<NA, NZ, TAB>(p, a, L, row, lane, sc BWD_STAMP_ARGS);
}

template <int NA, int NZ, bool TAB>
__device__ __forceinline__ void forward_compute(const AevParams& p, const AevArgs& a, FastLds& L, int row, int lane,
                                                StreamCur sc BWD_STAMP_PARAMS) {
  constexpr int NR = 16, Q = 64 / NA;

  // ---- radial: per species group, lanes = (slot q, shift k) ----
  {
    const int q = lane >> 4, k = lane & 15;
    const float shf = fmaf((float)k, p.dShfR, p.ShfR0);
    const float c = -p.EtaR * kLog2e;
    for (int s = 0; s < p.S; s++) {
      const int b0 = L.rstart[s], b1 = L.rstart[s + 1];
      if (b1 <= b0) continue;
      float acc = 0.f, acc2 = 0.f;
      int t = b0 + q;
      for (; t + 4 < b1; t += 8) {   // two neighbours per trip: their LDS reads and exponentials overlap
        const float r0 = L.rr[t], r1 = L.rr[t + 4], f0 = L.rfc[t], f1 = L.rfc[t + 4];
        const float d0 = r0 - shf, d1 = r1 - shf;
        acc = fmaf(fexp2(c * d0 * d0), f0, acc);
        acc2 = fmaf(fexp2(c * d1 * d1), f1, acc2);
      }
      if (t < b1) {
        const float dr = L.rr[t] - shf;
        acc = fmaf(fexp2(c * dr * dr), L.rfc[t], acc);
      }
      acc = xor_sum<32>(xor_sum<16>(acc + acc2));   // row / half-wave swaps, no LDS round trip
      if (q == 0) L.row[s * NR + k] = 0.25f * acc;
    }
  }

  BWD_STAMP(3);   // radial
  // ---- angular ----
  int nbk = 0, total;
  bool tabbed = false;   // wave-uniform: this centre's slots come from the stream table
  if constexpr (TAB) tabbed = sc.on;
  if (tabbed) {
    total = sc.total;
  } else {
    total = build_bucket_table<NA, NZ>(p, lane, L, nbk);
    wave_sync();
  }
  BWD_STAMP(4);   // bucket table
  float acc[NZ];
#pragma unroll
  for (int z = 0; z < NZ; z++) acc[z] = 0.f;
  int cur_off = -1;
  const int la = lane % NA, lq = lane / NA;
  const float cA = -p.EtaA * kLog2e;

  // A bucket's sums over the 64 / NA slot lanes of each shift.  Cross-lane moves are the expensive vector instructions here
  // (tools/issue_probe.hip: a half-wave or row swap takes the issue time of ~5 fp32 FMAs, a DPP move of ~3), so the NZ values
  // are not reduced one by one (NZ x 3..4 levels): each swap level HALVES the number of values a lane carries -- the pair
  // (acc[i], acc[i + NZ/2]) goes through ONE v_permlane32_swap whose two results add up to the lower half-wave's total of
  // acc[i] in the lower lanes and the upper half-wave's total of acc[i + NZ/2] in the upper ones; the same with the row swap
  // -- and the lane bits above the shift index end up selecting the section: lane = (z, [spare bit,] shift).
  auto flush = [&]() {
    if (cur_off >= 0) {
      float t[NZ / 2];
#pragma unroll
      for (int i = 0; i < NZ / 2; i++) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i]), __float_as_uint(acc[i + NZ / 2]), false, false);
        t[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
      }
      float u[NZ / 4];
#pragma unroll
      for (int i = 0; i < NZ / 4; i++) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(t[i]), __float_as_uint(t[i + NZ / 4]), false, false);
        u[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
      }
      float v;
      if constexpr (NA == 8) {        // NZ = 4: lane = (z: 2 bits, spare bit 3, shift: 3 bits)
        v = xor_sum<8>(u[0]);
      } else {                        // NA = 4, NZ = 8: lane = (z: 3 bits, spare bit 2, shift: 2 bits)
        const bool odd = lane & 8;
        const float keep = odd ? u[1] : u[0], send = odd ? u[0] : u[1];
        v = keep + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(send), 0x128, 0xf, 0xf, true));   // row_ror:8
        v = xor_sum<4>(v);
      }
      if ((lane & NA) == 0) L.row[cur_off + la * NZ + (lane >> (NA == 8 ? 4 : 3))] = v;
    }
#pragma unroll
    for (int z = 0; z < NZ; z++) acc[z] = 0.f;
  };

  for (int base = 0; base < total; base += 64) {
    // phase 1: lane = pair
    int outoff;
    {
      int ia, ib;
      bool valid;
      if (tabbed) {   // the word requested a step ago; the next step's leaves now
        const unsigned w = sc.w0;
        if (base + 64 < total) sc.w0 = sc.wp[base + 64 + lane];
        ia = w & 0xff;
        ib = (w >> 8) & 0xff;
        outoff = p.radial_len + (int)((w >> 16) & 0xff) * (NA * NZ);
        valid = (w >> 24) & 1;
      } else {
        stream_pair(L, nbk, base + lane, ia, ib, outoff, valid);
      }
      const float4 A = L.ad[ia], B = L.ad[ib];
      const float dot = A.x * B.x + A.y * B.y + A.z * B.z;
      const float cth = 0.95f * dot * frcp(fmaxf(A.w * B.w, 1e-10f));
      const float sth = __builtin_amdgcn_sqrtf(fmaxf(1.f - cth * cth, 0.f));
      const float w = valid ? 2.f * L.afc[ia] * L.afc[ib] : 0.f;
      const float rho = 0.5f * (A.w + B.w);
      // 16-byte stores (a lane's NZ / NA factors are contiguous): scalar stores at a 16- or 32-byte lane stride would
      // be 4- and 8-way bank conflicts
      float t1[NZ], t2[NA];
#pragma unroll
      for (int z = 0; z < NZ; z++) {
        const float basez = fmaxf(0.5f * (1.f + cth * p.cosZ[z] + sth * p.sinZ[z]), 0.f);
        t1[z] = w * fexp2(p.Zeta * flog2(basez));
      }
      float dr = rho - p.ShfA0;   // equidistant shifts: one subtraction per step instead of a table of NA scalars
#pragma unroll
      for (int s = 0; s < NA; s++) {
        t2[s] = fexp2(cA * dr * dr);
        dr -= p.dShfA;
      }
#pragma unroll
      for (int z = 0; z < NZ; z += 4)
        *reinterpret_cast<float4*>(L.pf1 + lane * NZ + z) = make_float4(t1[z], t1[z + 1], t1[z + 2], t1[z + 3]);
#pragma unroll
      for (int s = 0; s < NA; s += 4)
        *reinterpret_cast<float4*>(L.pf2 + lane * NA + s) = make_float4(t2[s], t2[s + 1], t2[s + 2], t2[s + 3]);
    }
    wave_sync();
    // phase 2: lane = (slot lq, shift la); group g covers slots g*Q .. g*Q+Q-1, all of one bucket (its output offset is
    // read from the register of the group's first pair: no LDS round trip in front of the flush test).  The factors of
    // group g+1 are requested before group g is accumulated.
    const int ngroups = min(NA, (total - base + Q - 1) / Q);
    float f2n = L.pf2[lq * NA + la];
    float4 qn[NZ / 4];
#pragma unroll
    for (int z4 = 0; z4 < NZ / 4; z4++) qn[z4] = *reinterpret_cast<const float4*>(L.pf1 + lq * NZ + 4 * z4);
#pragma unroll
    for (int g = 0; g < NA; g++) {
      if (g < ngroups) {   // wave-uniform
        const float f2 = f2n;
        float4 q[NZ / 4];
#pragma unroll
        for (int z4 = 0; z4 < NZ / 4; z4++) q[z4] = qn[z4];
        if (g + 1 < NA && g + 1 < ngroups) {
          const int slot = (g + 1) * Q + lq;
          f2n = L.pf2[slot * NA + la];
#pragma unroll
          for (int z4 = 0; z4 < NZ / 4; z4++) qn[z4] = *reinterpret_cast<const float4*>(L.pf1 + slot * NZ + 4 * z4);
        }
        const int off = __builtin_amdgcn_readlane(outoff, g * Q);
        if (off != cur_off) { flush(); cur_off = off; }
#pragma unroll
        for (int z4 = 0; z4 < NZ / 4; z4++) {
          acc[4 * z4] = fmaf(f2, q[z4].x, acc[4 * z4]); acc[4 * z4 + 1] = fmaf(f2, q[z4].y, acc[4 * z4 + 1]);
          acc[4 * z4 + 2] = fmaf(f2, q[z4].z, acc[4 * z4 + 2]); acc[4 * z4 + 3] = fmaf(f2, q[z4].w, acc[4 * z4 + 3]);
        }
      }
    }
    wave_sync();
  }
  flush();
  wave_sync();
  BWD_STAMP(5);   // angular

  float4* dst = reinterpret_cast<float4*>(a.aev + (long long)row * p.aev_stride);
  const int n4 = p.aev_stride >> 2;
  for (int e = lane; e < n4; e += 64) dst[e] = reinterpret_cast<const float4*>(L.row)[e];
  wave_sync();  // the LDS slice is reused by this wave's next centre
  BWD_STAMP(6);   // row store
}

// TBP: empty, or StreamTab for the instantiations that take slot words from the stream tables -- a parameter pack, so that the kernels
// without tables keep their argument list, and with it their instruction stream, exactly as it was
template <typename... TBP>
__device__ __forceinline__ StreamTab tab_of(const TBP&... tbp) {
  StreamTab t{};
  if constexpr (sizeof...(TBP) > 0) t = (tbp, ...);
  return t;
}

template <int NA, int NZ, int NCH, typename... TBP>
__global__ __launch_bounds__(64 * kWaves, kFwdMinWaves) void aev_forward_fast(AevParams p, AevArgs a, int cap, int rowf, TBP... tbp) {
  constexpr bool TAB = sizeof...(TBP) > 0;
  const StreamTab tab = tab_of(tbp...);
  extern __shared__ float4 smem4[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  FastLds L = carve<NA, NZ>(reinterpret_cast<float*>(smem4) + wave * fast_wave_floats_row(cap, false, rowf, p.S), cap, false, rowf);
#ifdef ABLB_STAMPS
  unsigned long long stamp_prev, stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_prev)::"memory");
  const int nw = gridDim.x * kWaves;
  for (int k = blockIdx.x * kWaves + wave; k < a.kcount; k += nw) {
    const int row = ticket_row(a, k);
    const hdr_t hc = load_header(a, row);
    BWD_STAMP(0);
    if (hc[0] < 0) continue;
    Loaded<NCH, false, 1> cur;
    load_lists(p, a, row, hdr_nrad(hc), hdr_nang(hc), lane, cur);
    BWD_STAMP(1);
    forward_centre<NA, NZ, NCH, TAB>(p, a, L, row, hc, cur, lane, tab, stamp_prev, stamp_acc);
    stamp_acc[7] += 1;
  }
  if (wave == 0 && lane == 0) {
    for (int q = 0; q < 7; q++) atomicAdd(&g_bwd_stamps[16 + q], stamp_acc[q]);
    atomicAdd(&g_bwd_stamps[24], stamp_acc[7]);
  }
#else
  ANI_PERSISTENT_LOOP(kWaves, NCH, false, 1, (forward_centre<NA, NZ, NCH, TAB>(p, a, L, row, hc, cur, lane, tab)))
#endif
}

// ---- the forward pass with the per-step compaction inside ("aev_fused") ----------------------------------------------------
// nbr_compact_kernel is bound by latency (list -> positions -> stores, little arithmetic: 0.09 ms at 100 000 centres at a third
// of the memory system's rate), aev_forward_fast by vector issue; run one after the other, each leaves the other's resource
// idle.  Here the wave that computes a centre's AEV row screens its candidate list itself: the gathers of the centre in hand
// are covered by the arithmetic of the five other waves of the SIMD, the descriptor and the candidate indices of the wave's
// NEXT centre travel during the arithmetic of this one (three registers), the LDS lists are filled straight from the
// screened candidates (no compact list read back, no unpack from it), and the compact list and its header are still
// written -- the backward kernel starts from them.  Candidate lists longer than 64 NCHC entries, or AEV shapes off the fast
// path, take the two kernels.
template <int NA, int NZ, int NCHC, typename... TBP>
__global__ __launch_bounds__(64 * kWaves, kFusedMinWaves) void aev_forward_fused(AevParams p, AevArgs a, int cap, int rowf, TBP... tbp) {
  constexpr bool TAB = sizeof...(TBP) > 0;
  const StreamTab tab = tab_of(tbp...);
  extern __shared__ float4 smem4[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  FastLds L = carve<NA, NZ>(reinterpret_cast<float*>(smem4) + wave * fast_wave_floats_row(cap, false, rowf, p.S), cap, false, rowf);
  ANI_TICKETS_BEGIN(kWaves)   // rows by ticket (see ANI_PERSISTENT_LOOP)
  const int cap2 = a.cl_stride - kMaxAng;   // room of the radial-only stream
  const float half_inv_Rcr = 0.5f * p.pi_over_Rcr * 0.3183098861837907f;  // r/(2 Rcr) revolutions
  const float half_inv_Rca = 0.5f * p.pi_over_Rca * 0.3183098861837907f;
  int4 info = load_info(a, k);
  int jj[NCHC];
  load_j(a, info, lane, jj);
  while (k < kend) {   // a group's rows are contiguous here (interleaved with the other groups' they run no faster or slower)
    ANI_TICKET_DRAW(tn)
    const int4 info1 = load_info(a, k1);       // in flight beside the gathers
    float4 xi, xx[NCHC];
    gather_x(a, info, jj, xi, xx);
    int jj1[NCHC];
    load_j(a, info1, lane, jj1);               // needs info1 only: the gathers stay in flight
    const int4 inf = uniform4(info);
    const int row = inf.w, i = inf.x, n = inf.x < 0 ? 0 : inf.z;
    for (int e = lane; e < (p.aev_stride >> 2); e += 64) reinterpret_cast<float4*>(L.row)[e] = make_float4(0, 0, 0, 0);
    int4* hdr = a.cl_hdr + 2 * (size_t)row;
    float4* oxyz = a.cl_xyz + (size_t)row * a.cl_stride;
    int* oj = a.cl_j + (size_t)row * a.cl_stride;
    // ---- screen (as nbr_compact_kernel): two append-only streams, per-species counts in lane s ----
    int nA = 0, nR = 0;
    int cc = 0;      // lane s: entries of species s in the angular stream (low half) and in the radial-only stream (high half)
    int spc[NCHC];   // the candidate's (compact) species
    float4 dd[NCHC];
    int pos[NCHC];   // slot in the row's compact list: [0, kMaxAng) angular stream, kMaxAng + .. radial-only stream, -1 screened out
#pragma unroll
    for (int c = 0; c < NCHC; c++) {
      pos[c] = -1;
      spc[c] = 0;
      dd[c] = make_float4(0.f, 0.f, 0.f, 1.f);
      if (64 * c < n) {   // wave-uniform
        const bool valid = 64 * c + lane < n;
        const float4 xj = xx[c];
        float4 d;
        d.x = xj.x - xi.x; d.y = xj.y - xi.y; d.z = xj.z - xi.z;
        d.w = __builtin_amdgcn_sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
        const int sp = __float_as_int(xj.w);
        const bool in_a = valid && d.w <= p.Rca;
        const bool in_2 = valid && !in_a && (p.compat || d.w <= p.Rcr);
        const unsigned long long mA = __ballot(in_a), m2 = __ballot(in_2);
        const int pA = nA + lanes_below(mA), p2 = nR + lanes_below(m2);
        for (int s = 0; s < p.S; s++) {
          const unsigned long long ms = __ballot(sp == s);
          const int k12 = __popcll(mA & ms) | (__popcll(m2 & ms) << 16);
          if (lane == s) cc += k12;
        }
        nA += __popcll(mA);
        nR += __popcll(m2);
        spc[c] = sp;
        dd[c] = d;
        pos[c] = (in_a && pA < kMaxAng) ? pA : ((in_2 && p2 < cap2) ? kMaxAng + p2 : -1);
      }
    }
    // stream table: the screened counts (lanes 0 and 1) -> tuple -> descriptor and first slot word, requested here, in front of the
    // centre's stores in the in-order memory queue; a row that is skipped below (over) is above the tables' bound as well
    StreamCur sc;
    if constexpr (TAB) {
      const int c0 = __builtin_amdgcn_readlane(cc, 0) & 0xffff, c1 = __builtin_amdgcn_readlane(cc, 1) & 0xffff;
      const bool live = inf.x >= 0 && !(nA > kMaxAng || nR > cap2 || nA + nR > cap);
      sc = stream_begin<64>(tab.desc_f, tab.words_f, live ? stream_tuple(p, tab, c0, c1) : -1, lane);
    }
    // the next centre's candidate indices are in registers before this centre's stores enter the (in-order) memory queue
#pragma unroll
    for (int c = 0; c < NCHC; c++) touch(jj1[c]);
    ANI_TICKET_TAKE(k2)
    const bool over = nA > kMaxAng || nR > cap2 || nA + nR > cap;   // never a silent truncation: row skipped, flag raised
#pragma unroll
    for (int c = 0; c < NCHC; c++)
      if (pos[c] >= 0) { oxyz[pos[c]] = dd[c]; oj[pos[c]] = cl_pack(jj[c], spc[c]); }
    if (lane < 8) {
      reinterpret_cast<unsigned char*>(hdr)[8 + lane] = (unsigned char)(cc & 0xffff);
      reinterpret_cast<unsigned short*>(hdr)[8 + lane] = (unsigned short)(cc >> 16);
    }
    if (lane == 0) {
      reinterpret_cast<int*>(hdr)[0] = (over || inf.x < 0) ? -1 : i;
      reinterpret_cast<int*>(hdr)[1] = (nA + nR) | (nA << 16) | (__float_as_int(xi.w) << 24);
      if (over) atomicOr(a.err_flag, 1);
    }
    if (!over && inf.x >= 0) {
      // ---- LDS lists straight from the screened candidates.  The candidates come sorted by species, so a candidate's place
      // in the species-grouped radial list is its stream index plus ONE number of its species: an angular entry of species s
      // sits behind the radial-only entries of the species before it (exclusive prefix of the radial-only counts), a
      // radial-only entry behind the angular entries up to and including its own species (inclusive prefix of the angular
      // counts).  The prefixes are a three-level DPP scan over the lanes that hold the counts -- no scalar tables (unpack_lists
      // walks 27 of them, which here spilled) -- and a candidate fetches its species' pair with one ds_bpermute. ----
      int inc = cc;
      inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xf, 0xf, true);   // row_shr:1
      inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xf, 0xf, true);   // row_shr:2
      inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xf, 0xf, true);   // row_shr:4
      const int exc = inc - cc;   // lane s: counts of the species before s; lane S: the totals
      if (lane <= p.S) { L.rstart[lane] = (exc & 0xffff) + (exc >> 16); L.astart[lane] = exc & 0xffff; }
      const int tab = (exc >> 16) | (inc << 16);   // {radial-only entries before species s, angular entries up to and including s}
#pragma unroll
      for (int c = 0; c < NCHC; c++) {
        const int t = __shfl(tab, spc[c]);
        if (pos[c] >= 0) {
          const bool ang = pos[c] < kMaxAng;
          const int w = ang ? pos[c] : pos[c] - kMaxAng;
          const int pr = w + (ang ? (t & 0xffff) : ((unsigned)t >> 16));
          const float4 v = dd[c];
          L.rr[pr] = v.w;
          L.rfc[pr] = 0.5f * fcos_rev(v.w * half_inv_Rcr) + 0.5f;
          if (ang) {
            L.ad[w] = v;
            L.afc[w] = 0.5f * fcos_rev(v.w * half_inv_Rca) + 0.5f;
          }
        }
      }
      wave_sync();
#ifdef ABLB_STAMPS
      unsigned long long stamp_prev = 0, stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      forward_compute<NA, NZ, TAB>(p, a, L, row, lane, sc, stamp_prev, stamp_acc);
#else
      forward_compute<NA, NZ, TAB>(p, a, L, row, lane, sc);
#endif
    }
    info = info1;
#pragma unroll
    for (int c = 0; c < NCHC; c++) jj[c] = jj1[c];
    ANI_TICKET_NEXT(tn, k2)
  }
  ANI_TICKETS_END(kWaves)
}

}  // namespace ani
