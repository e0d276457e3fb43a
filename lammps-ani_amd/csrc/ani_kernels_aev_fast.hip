// ani_kernels_aev_fast.hip — the forward and the backward kernels of the AEV fast path (ani_aev_fwd.h, ani_aev_bwd.h) and their
// launchers.  One translation unit for both: compiled apart from the backward kernels, the six aev_forward_fused instances with
// stream tables came out with three register copies in another order than before the split (profiles/aev_kernel_split_notes.md).
#include "ani_aev_launch.h"

#ifdef ABLB_STAMPS
namespace ani { __device__ unsigned long long g_bwd_stamps[32]; }   // backward: entries 0..8, forward: 16..24 (BWD_STAMP)
#endif
#include "ani_aev_fwd.h"
#include "ani_aev_bwd.h"

namespace ani {

int aev_read_stamps(unsigned long long* out32, int reset) {
#ifdef ABLB_STAMPS
  if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_bwd_stamps), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[32] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_bwd_stamps), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 2;
#else
  (void)out32; (void)reset;
  return 0;
#endif
}

// the forward kernels: the instance with the stream tables among its arguments, or the one without
template <typename K, typename KT>
static void launch_forward(K plain, KT tabbed, const AevParams& p, const AevArgs& a, const FastPlan& pl, hipStream_t st,
                           const StreamTab* tab) {
  const size_t lds = (size_t)fast_wave_floats_row(pl.cap, false, pl.rowf, p.S) * 4 * kWaves;
  if (tab) launch_fast(tabbed, p, a, kWaves, lds, pl.cap, pl.rowf, st, *tab);
  else launch_fast(plain, p, a, kWaves, lds, pl.cap, pl.rowf, st);
}

void launch_aev_forward(const AevParams& p, const AevArgs& a, int max_numneigh, hipStream_t st, const StreamTab* tab) {
  tab = usable_tab(p, tab);
  if (a.nrows <= 0) return;
  const FastPlan pl = fast_plan(p, max_numneigh);
  if (!pl.fast()) return launch_aev_forward_generic(p, a, st);
  if (a.kcount <= 0) return;   // an empty range of rows
  // 64-entry chunks of the radial-only stream prefetched per centre: 1 with the radial screen on (more than 64
  // neighbours between Rca and Rcr are loaded in place), 3 in pyaev mode where every candidate stays
  dispatch([&](auto K, auto NCH) {
    constexpr int NA = kGridNA<K>, NZ = kGridNZ<K>;
    launch_forward(aev_forward_fast<NA, NZ, NCH>, aev_forward_fast<NA, NZ, NCH, StreamTab>, p, a, pl, st, tab);
  }, one_of<1, 2>{pl.kind}, one_of<1, 3>{p.compat ? 3 : 1});
}

// compaction + forward in one launch; false: not applicable (the caller launches the two kernels)
bool launch_aev_forward_fused(const AevParams& p, const AevArgs& a, int max_numneigh, hipStream_t st, const StreamTab* tab) {
  const FastPlan pl = fast_plan(p, max_numneigh);
  if (a.nrows <= 0 || a.kcount <= 0 || !pl.fast() || max_numneigh > 256) return false;
  tab = usable_tab(p, tab);
  dispatch([&](auto K, auto NCHC) {
    constexpr int NA = kGridNA<K>, NZ = kGridNZ<K>;
    launch_forward(aev_forward_fused<NA, NZ, NCHC>, aev_forward_fused<NA, NZ, NCHC, StreamTab>, p, a, pl, st, tab);
  }, one_of<1, 2>{pl.kind}, one_of<2, 3, 4>{pl.chunks});
  return true;
}

bool launch_aev_backward(const AevParams& p, const AevArgs& a, int max_numneigh, hipStream_t st, const RepTab* rep, float* avir,
                         const StreamTab* tab) {
  if (a.nrows <= 0) return true;
  tab = usable_tab(p, tab);
  RepTab rt{};
  if (rep) rt = *rep;
  const FastPlan pl = fast_plan(p, max_numneigh);
  if (!pl.fast()) {
    launch_aev_backward_generic(p, a, st, avir);
    return false;
  }
  if (a.kcount <= 0) return true;
  const size_t lds = (size_t)bwd_wave_floats(pl.cap, pl.rowf, p.S, avir != nullptr) * 4 * kWavesB;
  auto go = [&](auto kernel, auto... extra) { launch_fast(kernel, p, a, kWavesB, lds, pl.cap, pl.rowf, st, rt, extra...); };
  // NCH as in the forward pass; GR: float4s of the dE/dAEV row a lane holds (rows of at most 256 floats: one).  Armed (per-atom
  // virial): its own instantiations, always with the global virial; the unarmed kernels stay what they were
  dispatch([&](auto K, auto NCH, auto GR, auto V) {
    constexpr int NA = kGridNA<K>, NZ = kGridNZ<K>;
    constexpr bool VIR = V != 0;
    if constexpr (GR == 1 && NCH == 1) {   // what a layout of one or two species runs with the radial screen on
      if (tab && !avir) return go(aev_backward_fast<NA, NZ, NCH, GR, VIR, StreamTab>, *tab);
    }
    if constexpr (VIR) {
      if (avir) return go(aev_backward_fast<NA, NZ, NCH, GR, true, float*>, avir);
    }
    go(aev_backward_fast<NA, NZ, NCH, GR, VIR>);
  }, one_of<1, 2>{pl.kind}, one_of<1, 3>{p.compat ? 3 : 1}, one_of<1, 4>{p.aev_stride <= 256 ? 1 : 4},
           one_of<0, 1>{avir || a.virial});
  return true;
}

}  // namespace ani
