// ani_fused_host.h — what the host needs to drive the fused MLP kernels (mlp_fused16 in ani_kernels_mlpg.hip, mlp_fused in
// ani_kernels_mlpf.hip): the table of compiled shapes, the sizes that follow from it, and the static schedule of a launch.
// Plain C++ -- no HIP, no environment -- compiled by the kernel files, by ani_hip_mlp.cpp and by stand-alone host programs
// (tests/ring_sim.cpp), like ani_fused_ring.h.  Internal to libani_hip.so.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace ani {

// 32-feature tiles of the three hidden layers (widths padded with zero weights), widest shape first.  The kernels' dispatch
// switches take their template arguments from here (the sixteen-row kernel counts 16-feature tiles: twice these).
constexpr int kNumFusedShapes = 3;
constexpr int kFusedShapes[kNumFusedShapes][3] = {{8, 6, 5}, {6, 5, 4}, {5, 4, 3}};

inline int fused_shape_for(int d1, int d2, int d3) {   // the narrowest shape that holds these widths; -1: none does
  for (int s = kNumFusedShapes - 1; s >= 0; s--)
    if (d1 <= 32 * kFusedShapes[s][0] && d2 <= 32 * kFusedShapes[s][1] && d3 <= 32 * kFusedShapes[s][2]) return s;
  return -1;
}
inline void fused_shape_tiles(int shape, int nt[3]) { for (int k = 0; k < 3; k++) nt[k] = kFusedShapes[shape][k]; }
// constants block of a member (floats): b0 | b1 | b2 | w3 padded to the shape's tiles, then {b3, 1/scale of the six products, 0}
inline int fused_consts_floats(int shape) {
  const int* s = kFusedShapes[shape];
  const int n = 32 * (s[0] + s[1] + 2 * s[2]) + 8;
  return (n + 255) / 256 * 256;   // whole 1 KB pieces
}
// 1 KB pieces of a member's weight stream: the 32-row kernel's (16-deep k-steps, 32-feature tiles) ...
inline long long fused_pieces_per_member(int shape, int acols, int P) {
  const int* s = kFusedShapes[shape];
  const long long ks0 = acols / 16, nt0 = (acols + 31) / 32;
  return P * (ks0 * s[0] + 2LL * s[0] * s[1] + 2LL * s[1] * s[2] + 2LL * s[2] * s[1] + 2LL * s[1] * s[0] + 2LL * s[0] * nt0);
}
// ... and the sixteen-row kernel's (32-deep k-steps, 16-feature tiles)
inline long long fused16_pieces_per_member(int shape, int acols, int P) {
  const int* s = kFusedShapes[shape];
  const long long n1 = 2 * s[0], n2 = 2 * s[1], n3 = 2 * s[2];
  const long long ks1 = (acols + 31) / 32, nt0 = (acols + 15) / 16;
  return P * (ks1 * n1 + (n1 / 2) * n2 + (n2 / 2) * n3 + n2 * (n3 / 2) + n1 * (n2 / 2) + nt0 * (n1 / 2));
}

// ---- static schedule of a launch -----------------------------------------------------------------------------------
// `ntypes` kinds of work items (type j: count[j] items of relative cost[j], items numbered type after type), `bins` workgroups.
// (Drawing items from a counter, costliest first, is list scheduling: at 100 002 water atoms -- 521 + 261 tiles of cost 1 and
// 0.67 on 256 CUs -- its last 14 tiles start when most CUs have finished, makespan 3.35; first-fit finds 3.0.)

// multifit: the smallest makespan T for which first-fit-decreasing packs every item; take[b * ntypes + j] = items of type j in bin b
inline double fused_pack(int ntypes, const int* count, const double* cost, int bins, std::vector<int>& best) {
  std::vector<int> order(ntypes);
  for (int j = 0; j < ntypes; j++) order[j] = j;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
  double total = 0.0, cmax = 0.0;
  for (int j = 0; j < ntypes; j++) { total += count[j] * cost[j]; if (count[j] > 0) cmax = std::max(cmax, cost[j]); }
  std::vector<int> take((size_t)bins * ntypes);
  auto fits = [&](double T) {
    std::fill(take.begin(), take.end(), 0);
    std::vector<double> rem(bins, T);
    for (int jj = 0; jj < ntypes; jj++) {
      const int j = order[jj];
      int left = count[j];
      if (left == 0 || cost[j] <= 0.0) { if (left) { take[j] += left; } continue; }
      for (int b = 0; b < bins && left > 0; b++) {
        const int k = std::min(left, (int)((rem[b] + 1e-9) / cost[j]));
        if (k > 0) { take[(size_t)b * ntypes + j] = k; rem[b] -= k * cost[j]; left -= k; }
      }
      if (left > 0) return false;
    }
    return true;
  };
  double lo = std::max(total / bins, cmax), hi = lo;
  while (!fits(hi)) hi *= 1.25;
  best = take;
  for (int it = 0; it < 24 && hi - lo > 1e-3 * hi; it++) {
    const double mid = 0.5 * (lo + hi);
    if (fits(mid)) { hi = mid; best = take; } else lo = mid;
  }
  return hi;
}

// items_out[sum count]: item numbers, workgroup after workgroup; off_out[bins + 1].  Returns the makespan.
inline double fused_schedule(int ntypes, const int* count, const double* cost, int bins, int* items_out, int* off_out) {
  std::vector<int> best, first(ntypes + 1, 0), order(ntypes);
  for (int j = 0; j < ntypes; j++) { order[j] = j; first[j + 1] = first[j] + count[j]; }
  std::sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
  const double T = fused_pack(ntypes, count, cost, bins, best);
  std::vector<int> next(first.begin(), first.end() - 1);
  int n = 0;
  for (int b = 0; b < bins; b++) {
    off_out[b] = n;
    for (int jj = 0; jj < ntypes; jj++) {
      const int j = order[jj];
      for (int k = 0; k < best[(size_t)b * ntypes + j]; k++) items_out[n++] = next[j]++;
    }
  }
  off_out[bins] = n;
  return T;
}

// The same with HALF items (the sixteen-row kernel: item total + 2 i + h = half h of item i, run by the lower half of a
// workgroup's waves at half_ratio of the item's cost -- more than half: the weights stream through the workgroup all the same).
// The last split[j] items of type j are cut in two where that shortens the schedule: the items beyond the last full round of
// workgroups otherwise make a round of their own with most of the chip idle.  split_mode 1: searched (a few candidate counts per
// type, most expensive types first, two sweeps; kept only if the makespan falls by min_gain -- the cost model is good to about
// 5 %: the caller either asks for 8 % or times the candidate against the whole items), 2: every item (tests, measurements).
// forced_split (experiments; null: none) overrides the mode: forced_split[j] in [0, count[j]] of type j's last items are cut.
// items_out holds up to sum(count) + max splits entries.  Returns the makespan; *n_items_out = entries written.
inline double fused_schedule_halves(int ntypes, const int* count, const double* cost, double half_ratio, int bins, int split_mode,
                                    const int* forced_split, int* split_out, int* items_out, int* off_out, int* n_items_out,
                                    double min_gain = 0.08) {
  std::vector<int> first(ntypes + 1, 0);
  for (int j = 0; j < ntypes; j++) first[j + 1] = first[j] + count[j];
  const int total = first[ntypes];
  std::vector<int> split(ntypes, 0), ecount(2 * ntypes), best;
  std::vector<double> ecost(2 * ntypes);
  for (int j = 0; j < ntypes; j++) { ecost[j] = cost[j]; ecost[ntypes + j] = half_ratio * cost[j]; }
  auto makespan = [&](const std::vector<int>& sp, std::vector<int>& take) {
    for (int j = 0; j < ntypes; j++) { ecount[j] = count[j] - sp[j]; ecount[ntypes + j] = 2 * sp[j]; }
    return fused_pack(2 * ntypes, ecount.data(), ecost.data(), bins, take);
  };
  double T = makespan(split, best);
  if (forced_split) {
    split.assign(forced_split, forced_split + ntypes);
    T = makespan(split, best);
  } else if (split_mode == 2) {
    for (int j = 0; j < ntypes; j++) split[j] = count[j];
    T = makespan(split, best);
  } else if (split_mode == 1) {
    const double T0 = T;
    std::vector<int> order(ntypes), cur = split, take;
    for (int j = 0; j < ntypes; j++) order[j] = j;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] * count[a] > cost[b] * count[b]; });
    double Tc = T;
    for (int sweep = 0; sweep < 2; sweep++)
      for (int jj = 0; jj < ntypes && jj < 4; jj++) {
        const int j = order[jj];
        if (count[j] == 0) continue;
        const int cap = std::min(count[j], bins);
        const int cand[7] = {0, count[j] % bins, cap / 8, cap / 4, cap / 2, (3 * cap) / 4, cap};
        int keep = cur[j];
        for (int c : cand) {
          if (c < 0 || c > count[j]) continue;
          std::vector<int> trial = cur;
          trial[j] = c;
          const double Tt = makespan(trial, take);
          if (Tt < Tc * (1.0 - 1e-6)) { Tc = Tt; keep = c; }
        }
        cur[j] = keep;
      }
    if (Tc < (1.0 - min_gain) * T0) { split = cur; T = makespan(split, best); }
    else T = makespan(split, best);
  }
  // numbering: type j's whole items first[j] .. first[j] + count[j] - split[j]; the halves of the split[j] items behind them
  std::vector<int> order(2 * ntypes), next(2 * ntypes, 0);
  for (int j = 0; j < 2 * ntypes; j++) order[j] = j;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return ecost[a] > ecost[b]; });
  int n = 0;
  for (int b = 0; b < bins; b++) {
    off_out[b] = n;
    for (int jj = 0; jj < 2 * ntypes; jj++) {
      const int e = order[jj];
      for (int k = 0; k < best[(size_t)b * 2 * ntypes + e]; k++) {
        const int i = next[e]++;
        if (e < ntypes) items_out[n++] = first[e] + i;
        else {
          const int j = e - ntypes;
          items_out[n++] = total + 2 * (first[j] + count[j] - split[j] + (i >> 1)) + (i & 1);
        }
      }
    }
  }
  off_out[bins] = n;
  if (split_out) for (int j = 0; j < ntypes; j++) split_out[j] = split[j];
  if (n_items_out) *n_items_out = n;
  return T;
}

}  // namespace ani
