// ani_aev_launch.h — host side of the AEV launches, shared by ani_kernels_aev_{lists,fast}.hip: which path a model takes,
// the LDS capacity of a launch, the persistent grid.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

#include "ani_aev_device.h"

namespace ani {

inline int fast_kind(const AevParams& p) {
  if (p.nR != 16 || p.S > 8 || (p.aev_stride & 3) || !p.equi) return 0;
  {
    // the backward kernel's radial Gaussians come from a recurrence around the midpoints of the two halves of the shifts
    // (backward_centre): its ratio H^2 = exp(2 EtaR dc Delta) must stay inside fp32 for every r in (0, Rcr], 1 / C_3.5 =
    // exp(EtaR (3.5 Delta)^2) too, and where E = exp(-EtaR dc^2) underflows the half's largest term must be negligible.
    // Parameter sets beyond that take the generic kernels.
    const float d = fabsf(p.dShfR), c0 = p.ShfR0 + 3.5f * p.dShfR, c1 = p.ShfR0 + 11.5f * p.dShfR;
    const float dmax = fmaxf(fmaxf(fabsf(p.Rcr - c0), fabsf(c0)), fmaxf(fabsf(p.Rcr - c1), fabsf(c1)));
    const float q = sqrtf(87.f / p.EtaR) - 3.5f * d;
    if (2.f * p.EtaR * dmax * d > 80.f || p.EtaR * 12.25f * d * d > 80.f || q <= 0.f || p.EtaR * q * q < 20.f) return 0;
  }
  if (p.nA == 8 && p.nZ == 4) return 1;
  if (p.nA == 4 && p.nZ == 8) return 2;
  return 0;
}

// Capacity of the per-centre radial list in LDS.  pyaev semantics keep every list entry, so the longest list decides.
// With the radial screen at Rcr only the entries inside Rcr are kept -- for the reference's settings (5.1 A inside a
// 7.1 A list) 37 % of a uniform neighbourhood -- so 3/4 of the longest list (at least 128 slots) is reserved instead of
// all of it; the smaller LDS slice is what lets more waves share a CU.  A centre that still overflows raises the
// capacity error like any other overflow (never a silent truncation), and AevParams::full_cap restores the full size.
// The capacity is rounded up to kCapGrain slots; 32 (a fifth forward workgroup per CU) measured slower: 0.246 against 0.230 ms.
constexpr int kCapGrain = 64;
inline int radial_cap(const AevParams& p, int max_numneigh) {
  int full = (max_numneigh + 63) / 64 * 64;
  if (full < 64) full = 64;
  if (p.compat || p.full_cap) return full;
  int est = (3 * max_numneigh + 3) / 4;
  if (est < 128) est = 128;
  est = (est + kCapGrain - 1) / kCapGrain * kCapGrain;
  return est < full ? est : full;
}

// What a launch of the AEV kernels does, decided in one place from the model's parameters and the longest candidate list; every
// launcher and aev_fast_path / aev_compact_stride read it.
struct FastPlan {
  int kind;     // 0: the generic kernels; fast path with the angular grid NA x NZ = 8x4 (1) or 4x8 (2)
  int cap;      // LDS capacity of a centre's radial list (radial_cap)
  int rowf;     // LDS floats of an AEV row: the row stride rounded up to 64
  int chunks;   // 64-entry chunks of a candidate list that the compaction holds in registers: 2, 3 or 4 (longer lists: in place)
  bool fits;    // a backward workgroup (kWavesB slices) and a forward workgroup (kWaves slices) each fit in 160 KB
  bool fast() const { return kind != 0 && fits; }
};
inline FastPlan fast_plan(const AevParams& p, int max_numneigh) {
  FastPlan f{};
  f.kind = fast_kind(p);
  f.cap = radial_cap(p, max_numneigh);
  f.rowf = (p.aev_stride + 63) / 64 * 64;
  f.chunks = max_numneigh <= 128 ? 2 : (max_numneigh <= 192 ? 3 : 4);
  f.fits = (size_t)fast_wave_floats(f.cap, true) * 4 * kWavesB <= 160 * 1024 &&
           (size_t)fast_wave_floats(f.cap, false) * 4 * kWaves <= 160 * 1024;
  return f;
}

// Runtime choices -> template arguments.  dispatch(f, one_of<1, 2>{kind}, one_of<1, 3>{nch}) calls f(c1, c2) with each value as a
// std::integral_constant, so that a generic lambda can name the kernel instance; a value outside its list calls nothing.  f is
// instantiated for every combination of the lists: the kernels that exist are the ones its body names for a combination (a
// kernel that only some combinations have stands under an if constexpr).
template <int... Vs>
struct one_of { int v; };
template <typename F>
void dispatch(F&& f) { f(); }
template <typename F, int... Vs, typename... Rest>
void dispatch(F&& f, one_of<Vs...> c, Rest... rest) {
  (void)((c.v == Vs && (dispatch([&](auto... k) { f(std::integral_constant<int, Vs>{}, k...); }, rest...), true)) || ...);
}
// the angular grid of a kind
template <int KIND> constexpr int kGridNA = KIND == 1 ? 8 : 4;
template <int KIND> constexpr int kGridNZ = KIND == 1 ? 4 : 8;

inline const char* waves_env() { return "ANI_AEV_WAVES_PER_CU"; }  // experiment knob: cap on resident waves per CU
// persistent grid of the fast path: as many workgroups as fit on the chip by LDS (at most 8 per CU)
template <typename K>
static int persistent_blocks(K kernel, int nrows, int waves_per_block, size_t lds_bytes) {
  // resident workgroups per CU by registers AND LDS; a grid larger than what is resident would run a second,
  // mostly empty round of persistent workgroups
  // the occupancy query costs microseconds of host time per launch: asked once per (kernel, LDS size)
  static std::map<std::pair<const void*, size_t>, int> cache;
  static std::mutex mtx;
  int per_cu = 0;
  {
    std::lock_guard<std::mutex> lock(mtx);
    const auto key = std::make_pair((const void*)kernel, lds_bytes);
    const auto it = cache.find(key);
    if (it != cache.end()) per_cu = it->second;
    else {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64 * waves_per_block, lds_bytes) != hipSuccess || per_cu < 1)
        per_cu = (int)((160 * 1024) / (lds_bytes ? lds_bytes : 1));
      cache[key] = per_cu;
    }
  }
  if (per_cu > 8) per_cu = 8;
  static const int forced = [] { const char* e = getenv(waves_env()); return e ? atoi(e) : 0; }();
  if (forced > 0 && forced * waves_per_block / 2 >= 1) per_cu = std::min(per_cu, std::max(1, forced / waves_per_block));
  if (per_cu < 1) per_cu = 1;
  const int need = (nrows + waves_per_block - 1) / waves_per_block;
  const int fit = device_num_cus() * per_cu;
  return need < fit ? need : fit;
}

template <typename K, typename... Extra>
static void launch_fast(K kernel, const AevParams& p, const AevArgs& a, int waves, size_t lds, int cap, int rowf, hipStream_t st,
                        Extra... extra) {
  note_launch_error(raise_dynamic_lds((const void*)kernel, 160 * 1024));
  hipLaunchKernelGGL(kernel, dim3(persistent_blocks(kernel, a.kcount, waves, lds)), dim3(64 * waves), lds, st, p, a, cap, rowf,
                     extra...);
}

// tables only where they were built for this layout: one or two species
inline const StreamTab* usable_tab(const AevParams& p, const StreamTab* tab) {
  return (tab && tab->desc_b && tab->desc_f && (p.S == 1 || p.S == 2)) ? tab : nullptr;
}

// the first-generation kernels of ani_kernels_aev_generic.hip, for the model shapes off the fast path
void launch_aev_forward_generic(const AevParams& p, const AevArgs& a, hipStream_t st);
void launch_aev_backward_generic(const AevParams& p, const AevArgs& a, hipStream_t st, float* avir);

}  // namespace ani
