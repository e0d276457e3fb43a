// ani_aev_stream.h — the angular pair streams of the AEV fast path and the persistent row loop: bucket and pair tables, the
// arithmetic slot decodes, a centre's place in the stream tables (StreamTab in ani_kernels.h), the row tickets.
#pragma once
#include "ani_aev_device.h"

namespace ani {

// Build the table of non-empty species-pair buckets.  Returns the padded stream length; nbk = number of entries.
// entry: {tstart, a1, n1, a2, n2, outoff, tri, npairs}
template <int NA, int NZ>
__device__ __forceinline__ int build_bucket_table(const AevParams& p, int lane, FastLds& L, int& nbk) {
  constexpr int Q = 64 / NA;
  const int nb_all = p.S * (p.S + 1) / 2;
  int s1 = 0, s2 = 0, np = 0, n1 = 0, n2 = 0;
  if (lane < nb_all) {
    int rem = lane;
    while (rem >= p.S - s1) { rem -= p.S - s1; s1++; }
    s2 = s1 + rem;
    n1 = L.astart[s1 + 1] - L.astart[s1];
    n2 = L.astart[s2 + 1] - L.astart[s2];
    np = (s1 == s2) ? n1 * (n1 - 1) / 2 : n1 * n2;
  }
  const int npad = (np + Q - 1) / Q * Q;
  const int incl = wave_incl_scan(npad);
  const unsigned long long m = __ballot(np > 0);
  if (np > 0) {
    int* e = L.tb + 8 * lanes_below(m);
    e[0] = incl - npad; e[1] = L.astart[s1]; e[2] = n1; e[3] = L.astart[s2]; e[4] = n2;
    e[5] = p.radial_len + lane * (NA * NZ); e[6] = (s1 == s2) ? 1 : 0; e[7] = np;
  }
  nbk = __popcll(m);
  return __builtin_amdgcn_readlane(incl, 63);
}

// lane -> its pair of the padded stream.  valid = false for padding slots (indices then point at neighbour 0 of
// the group, a harmless geometry).
__device__ __forceinline__ void stream_pair(const FastLds& L, int nbk, int t, int& ia, int& ib, int& outoff, bool& valid) {
  int e = 0;
  for (int k = 1; k < nbk; k++)
    if (t >= L.tb[8 * k]) e = k;
  const int4 e0 = *reinterpret_cast<const int4*>(L.tb + 8 * e);
  const int4 e1 = *reinterpret_cast<const int4*>(L.tb + 8 * e + 4);
  const int u = t - e0.x;
  valid = u < e1.w;
  outoff = e1.y;
  int a = 0, b = 0;
  if (valid) {
    if (e1.z) {
      decode_pair(u, e0.z, a, b);
    } else {
      a = (int)(((float)u + 0.5f) * frcp((float)e1.x));
      b = u - a * e1.x;
    }
  } else if (e1.z) {
    b = 1;  // distinct neighbours keep the padded geometry finite
  }
  ia = e0.y + a;
  ib = e0.w + b;
}

// Backward, dense pair stream in two half-waves.  Lanes 0..31 and 32..63 walk the SAME sequence of 32 "column slots" per
// step, the lower half on the even row neighbours of a bucket, the upper half on the odd ones: lane l and lane l + 32 hold
// pairs (a, b) and (a + 1, b) with the same column neighbour b, so a column's gradient leaves the step as ONE LDS add per two
// pairs (the two halves are summed with a half-wave swap; LDS float adds cost about a cycle per active lane, and at one add
// per pair they made the LDS, not the vector unit, the busiest part of the CU).  Rows come in BANDS of two: a rectangular
// bucket (n1 rows x n2 columns; the larger species group is the columns) has ceil(n1 / 2) bands of n2 slots (an odd last row
// leaves its upper half idle); a triangular one (pairs a < b of n neighbours) has bands k = 0 .. n/2 - 1 of rows 2k, 2k + 1
// with n - 1 - 2k slots, column b = 2k + 1 + slot -- the upper half idles at slot 0, where its row meets itself -- floor(n^2/4)
// slots in all.  A water centre: 36 + 36 + 9 = 81 slots = 3 steps for its 153 pairs.
// Table entry: {vstart, ra, nr, ca, nc, outoff, tri, slots}; returns the number of slots.
template <int NA, int NZ>
__device__ __forceinline__ int build_pair_table(const AevParams& p, int lane, FastLds& L, int& nbk) {
  const int nb_all = p.S * (p.S + 1) / 2;
  int s1 = 0, s2 = 0, ns = 0, n1 = 0, n2 = 0;
  bool sw = false;
  if (lane < nb_all) {
    int rem = lane;
    while (rem >= p.S - s1) { rem -= p.S - s1; s1++; }
    s2 = s1 + rem;
    n1 = L.astart[s1 + 1] - L.astart[s1];
    n2 = L.astart[s2 + 1] - L.astart[s2];
    if (s1 == s2) {
      ns = (n1 * n1) >> 2;                       // 0 for n1 < 2
    } else if (n1 > 0 && n2 > 0) {
      sw = n2 < n1;                              // rows = the smaller group
      const int nr = sw ? n2 : n1, nc = sw ? n1 : n2;
      ns = ((nr + 1) >> 1) * nc;
    }
  }
  const int incl = wave_incl_scan(ns);
  const unsigned long long m = __ballot(ns > 0);
  if (ns > 0) {
    int* e = L.tb + 8 * lanes_below(m);
    e[0] = incl - ns; e[1] = L.astart[sw ? s2 : s1]; e[2] = sw ? n2 : n1; e[3] = L.astart[sw ? s1 : s2]; e[4] = sw ? n1 : n2;
    e[5] = p.radial_len + lane * (NA * NZ); e[6] = (s1 == s2) ? 1 : 0; e[7] = ns;
  }
  nbk = __popcll(m);
  return __builtin_amdgcn_readlane(incl, 63);
}
// lane -> its pair: slot v of the stream, half h (0: the band's even row, 1: its odd row).  pos = the pair's position in its
// run (the consecutive lanes of a half-wave that share the row neighbour ia).  Idle lanes (past the end, an odd last row's
// upper half, the upper half at a triangular band's first slot): valid = false, pos = 0, and the indices of a harmless pair.
__device__ __forceinline__ void stream_pair_half(const FastLds& L, int nbk, int v, int h, int& ia, int& ib, int& outoff, int& pos,
                                                 bool& valid) {
  int e = 0;
  for (int k = 1; k < nbk; k++)
    if (v >= L.tb[8 * k]) e = k;
  const int4 e0 = *reinterpret_cast<const int4*>(L.tb + 8 * e);       // vstart, ra, nr, ca
  const int4 e1 = *reinterpret_cast<const int4*>(L.tb + 8 * e + 4);   // nc, outoff, tri, slots
  const int u = v - e0.x;
  outoff = e1.y;
  int a = 0, b = 0;
  pos = 0;
  valid = nbk > 0 && u < e1.w;
  if (valid) {
    if (e1.z) {
      // band k: the largest k with k (n - k) <= u; closed form + one correction step each way (all quantities < 2^14)
      const int n = e0.z;
      const float fn = (float)n;
      int k = (int)((fn - __builtin_amdgcn_sqrtf(fmaxf(fn * fn - 4.f * (float)u, 0.f))) * 0.5f);
      k = max(0, min(k, (n >> 1) - 1));
      if (__mul24(k, n - k) > u) k--;
      if (__mul24(k + 1, n - k - 1) <= u) k++;
      const int c = u - __mul24(k, n - k);
      a = 2 * k + h;
      b = 2 * k + 1 + c;
      pos = c - h;
      valid = h == 0 || c >= 1;
    } else {
      const int k = (int)(((float)u + 0.5f) * frcp((float)e1.x));
      const int c = u - k * e1.x;
      a = 2 * k + h;
      b = c;
      pos = c;
      valid = a < e0.z;
    }
  }
  if (!valid) { a = 0; b = e1.z ? 1 : 0; pos = 0; }   // two distinct neighbours of a non-empty bucket (a triangular one has n >= 2)
  ia = e0.y + a;
  ib = e0.w + b;
}

// ---- stream tables (StreamTab in ani_kernels.h): the two decodes above, done once per tuple of counts ----------------------
// A centre's place in its stream: where its lane reads its slot words, how long the stream is, and the words already requested.
// on = false: the centre decodes its slots arithmetically (no tables, or a count above their bound).
struct StreamCur {
  const unsigned* wp = nullptr;   // the stream's first word (wave-uniform: the lane adds its slot)
  int total = 0;                  // stream length (slots)
  unsigned w0 = 0, w1 = 0;        // the words of the next step and (backward) of the one after it
  bool on = false;
};
// tuple index of a centre with n0 / n1 angular neighbours of species 0 / 1, -1 above the tables' bound.  The counts are compared
// with the bound before they index anything.
__device__ __forceinline__ int stream_tuple(const AevParams& p, const StreamTab& t, int n0, int n1) {
  if (p.S == 1) return (unsigned)n0 <= (unsigned)t.nt ? n0 : -1;
  return ((unsigned)n0 <= (unsigned)t.nt && (unsigned)n1 <= (unsigned)t.nt) ? n0 * (t.nt + 1) + n1 : -1;
}
// the descriptor through the scalar cache (as load_header_scalar), then the first word(s): STEP = slots per step (64 forward: one
// word ahead; 32 backward, both half-waves on the same word: two ahead, the second step's word would otherwise be requested behind
// the radial-only scatter in the in-order memory queue)
template <int STEP>
__device__ __forceinline__ StreamCur stream_begin(const int4* desc, const unsigned* words, int tix, int lane) {
  StreamCur c;
  if (tix < 0) return c;   // wave-uniform
  int4 d;
  asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(d) : "s"(desc + tix) : "memory");
  c.on = true;
  c.total = d.y;
  c.wp = words + d.x;
  if (d.y > 0) c.w0 = c.wp[lane & (STEP - 1)];
  if (STEP == 32 && d.y > STEP) c.w1 = c.wp[STEP + (lane & 31)];
  return c;
}

// row of position kk of a launch's range (wave-uniform); a position past the end reads the last row
__device__ __forceinline__ int ticket_row(const AevArgs& a, int kk) {
  const int kc = kk < a.kcount ? kk : a.kcount - 1;
  return a.row_list ? __builtin_amdgcn_readfirstlane(a.row_list[a.k0 + kc]) : a.k0 + kc;
}

// Persistent waves: wave w handles rows w, w + W, w + 2W, ...  A centre's inputs (header, list chunks, dE/dAEV row: all
// addressed by the row alone) are requested when the centre is started and waited for on the spot: the kernels are
// bound by what their resident waves execute, not by one wave's latency, so the other waves cover the wait.  Requesting
// them one centre ahead (two register stages used alternately, secured before the centre's stores and atomics entered
// the in-order vmcnt queue) was built and measured: forward unchanged, backward 4 % SLOWER -- the second stage costs
// 22 registers that the pair loop uses better.
// Which rows a wave takes: by ticket when the launch has counters (AevArgs::row_counter) -- centres cost differently, and with a
// fixed stride a kernel ends with its unluckiest wave (forward pass with the compaction inside: 0.252 -> 0.224 ms) -- else a
// fixed stride.  The workgroups form kTicketGroups groups (blockIdx mod groups), each with a contiguous share of the rows and
// a counter of its own (ONE counter would serialise 100 000 same-address atomics: measured 1.3 ms).  A wave holds the tickets
// of its current and its next centre and has two more on their way: the one drawn a centre ago is taken behind the centre's
// first wait for loaded data, at no cost (the memory queue is in order).  A group's last wave out leaves the counters at zero for the next launch on the stream.
// The macros expect a, wave and lane in scope and declare in the kernel's scope (a struct with these as members was compiled: every
// kernel that used it came out with other code, profiles/aev_kernel_split_notes.md):
//   k, k1       positions in the launch's range of the wave's current and next centre -- a kernel body reads them, only
//               ANI_TICKET_NEXT changes them
//   kend, nw    where k stops (contiguous shares) and the stride without counters -- read only
//   tk_ctr, tk_ngrp, tk_grp, tk_share, tk_base   the group's counters and its share of the rows -- read only, and only by a kernel that
//               interleaves a group's rows with the other groups' (aev_backward_fast: rank_of, kstop)
//   tk_pending  lane 0's ticket on its way -- the macros' own
// ANI_TICKET_DRAW(tn) and ANI_TICKET_TAKE(k2) declare the two names they are given; ANI_TICKET_NEXT(tn, k2) takes them back.
#define ANI_TICKETS_BEGIN(KW)                                                                              \
  const int nw = gridDim.x * KW;                                                                          \
  const int tk_ngrp = min((int)gridDim.x, kTicketGroups), tk_grp = blockIdx.x % tk_ngrp;                  \
  const int tk_share = (a.kcount + tk_ngrp - 1) / tk_ngrp, tk_base = tk_grp * tk_share;                   \
  int* const tk_ctr = a.row_counter ? a.row_counter + kTicketStride * tk_grp : nullptr;                   \
  const int kend = tk_ctr ? min(a.kcount, tk_base + tk_share) : a.kcount;                                 \
  int k = blockIdx.x * KW + wave, k1 = k + nw, tk_pending = 0;                                            \
  if (tk_ctr) {                                                                                           \
    int t0 = 0, t1 = 0;                                                                                   \
    if (lane == 0) { t0 = atomicAdd(tk_ctr, 1); t1 = atomicAdd(tk_ctr, 1); tk_pending = atomicAdd(tk_ctr, 1); } \
    k = tk_base + __builtin_amdgcn_readfirstlane(t0);                                                     \
    k1 = tk_base + __builtin_amdgcn_readfirstlane(t1);                                                    \
  }
/* at the top of a centre: the ticket three centres ahead leaves ... */
#define ANI_TICKET_DRAW(tn)                                                                                \
  int tn = 0;                                                                                             \
  if (tk_ctr && lane == 0) tn = atomicAdd(tk_ctr, 1);
/* ... and behind the centre's first wait for loaded data (which, the memory queue being in order, is also a wait for everything
   the wave issued before): the ticket drawn a centre ago is taken into a scalar register */
#define ANI_TICKET_TAKE(k2)                                                                                \
  touch(tk_pending);                                                                                      \
  const int k2 = tk_base + __builtin_amdgcn_readfirstlane(tk_pending);
#define ANI_TICKET_NEXT(tn, k2)                                                                            \
  k = k1;                                                                                                 \
  k1 = tk_ctr ? k2 : k1 + nw;                                                                             \
  tk_pending = tn;
#define ANI_TICKETS_END(KW)                                                                                \
  if (tk_ctr && lane == 0 && atomicAdd(tk_ctr + 1, 1) == ((int)gridDim.x - tk_grp + tk_ngrp - 1) / tk_ngrp * KW - 1) { \
    __atomic_store_n(tk_ctr, 0, __ATOMIC_RELAXED);                                                        \
    __atomic_store_n(tk_ctr + 1, 0, __ATOMIC_RELAXED);                                                    \
  }
#define ANI_PERSISTENT_LOOP(KW, NCH, BWD, GR, CENTRE)                                                      \
  ANI_TICKETS_BEGIN(KW)                                                                                   \
  while (k < ((tk_ctr && BWD) ? tk_base + tk_share : kend)) {                                             \
    ANI_TICKET_DRAW(tk_tn)                                                                                \
    const int kk = (tk_ctr && BWD) ? (k - tk_base) * tk_ngrp + tk_grp : k;   /* backward: a group's rows interleaved with the others' */ \
    const int row = ticket_row(a, kk);                                                                    \
    const hdr_t hc = load_header(a, row);                                                                 \
    ANI_TICKET_TAKE(tk_k2)                                                                                \
    if (hc[0] >= 0 && kk < a.kcount) {                                                                    \
      Loaded<NCH, BWD, GR> cur;                                                                           \
      load_lists(p, a, row, hdr_nrad(hc), hdr_nang(hc), lane, cur);                                       \
      CENTRE;                                                                                             \
    }                                                                                                     \
    ANI_TICKET_NEXT(tk_tn, tk_k2)                                                                         \
  }                                                                                                       \
  ANI_TICKETS_END(KW)

}  // namespace ani
