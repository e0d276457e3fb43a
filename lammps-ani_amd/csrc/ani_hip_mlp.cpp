// ani_hip_mlp.cpp — host side of the MLP: activation arena, fused launch, per-layer launches.  Internal: see ani_handle.h.
#include "ani_handle.h"

namespace ani_host __attribute__((visibility("hidden"))) {
constexpr double kFusedHalfCost = 0.75;   // cost of a half item of the sixteen-row fused MLP relative to its whole item (measured 0.64 - 0.76)

// activation arena of the per-layer MLP kernels: per species, H_k (k = 1..L-1; H_{L-1} is overwritten by dE/dz_{L-1}) and
// the raw gradients dE/dh_k (k = 1..L-2), whose celu' factor is applied by the product that consumes them.  The fused
// kernel keeps all of this in registers: an epoch that only ever runs it never allocates or clears the arena.
int ensure_arena(ani_handle* h, hipStream_t st) {
  if (h->arena_valid) return ANI_OK;
  const HostModel& m = h->model;
  size_t need = 0;
  for (int s = 0; s < m.S; s++) {
    const size_t rows = round_up(h->count[s], kRowTile);
    for (int k = 1; k < m.L; k++) need += rows * (size_t)m.M * h->nets[s].w[k];
    for (int k = 1; k < m.L - 1; k++) need += rows * (size_t)m.M * h->nets[s].w[k];
  }
  HIP_TRY(h, h->act.reserve(std::max<size_t>(need, 1)));
  HIP_TRY(h, hipMemsetAsync(h->act.p, 0, need * sizeof(float), st));  // zero K-padding columns
  h->Hbuf.assign(m.S, std::vector<float*>(m.L, nullptr));
  h->Gbuf.assign(m.S, std::vector<float*>(m.L, nullptr));
  size_t off = 0;
  for (int s = 0; s < m.S; s++) {
    const size_t rows = round_up(h->count[s], kRowTile);
    for (int k = 1; k < m.L; k++) {
      h->Hbuf[s][k] = h->act.p + off;
      off += rows * (size_t)m.M * h->nets[s].w[k];
    }
    for (int k = 1; k < m.L - 1; k++) {
      h->Gbuf[s][k] = h->act.p + off;
      off += rows * (size_t)m.M * h->nets[s].w[k];
    }
  }
  h->arena_valid = true;
  return ANI_OK;
}

// ---- fused MLP: eligibility, stream construction, launch ---------------------------------------------------------
bool fused_eligible(const ani_handle* h) {
  const HostModel& m = h->model;
  if (!h->opt.mlp_fused || h->opt.mlp_arith == MLP_FP32 || m.L != 4) return false;
  // Small systems: a fused tile takes ~0.1 ms whatever else happens, so with fewer tiles than CUs the kernel costs that much
  // however few rows there are, while the chained per-layer launch of small systems scales down with them (MLP, exact
  // arithmetic: 12 501 atoms 0.09 fused against 0.08 chained; 25 002 atoms 0.09 against 0.12): fused from ~16 000 atoms on.
  if (h->opt.mlp_fused < 2 && m.M == 1 && !h->opt.mlp_fused_gen) {   // (several members: the fused kernel's (tile, member) work items win at every size measured)
    int tiles = 0;
    for (int s = 0; s < m.S; s++) tiles += round_up(h->count[s], kRowTile) / kRowTile;
    if (tiles < 125) return false;
  }
  const int acols = h->ap_run.aev_len;
  if (acols < 16 || (acols & 15) || (h->ap_run.aev_stride & 3)) return false;
  for (int s = 0; s < m.S; s++)
    if (fused_shape_for(m.dims[s][1], m.dims[s][2], m.dims[s][3]) < 0 || m.dims[s][4] != 1) return false;
  return true;
}

void free_fused(ani_handle* h, int fi) {
  for (auto& n : h->nets) {
    if (n.fu[fi].stream) (void)hipFree(n.fu[fi].stream);
    if (n.fu[fi].consts) (void)hipFree(n.fu[fi].consts);
    n.fu[fi] = SpeciesNet::Fused{};
  }
  h->fused.mask[fi] = -2;
}

// weight streams + constants of every species for arithmetic `arith`, in the AEV layout of this epoch
int ensure_fused(ani_handle* h, MlpArith arith, int gen, hipStream_t st) {
  const int pi = arith == MLP_F16X2 ? 1 : 0, P = mlp_planes(arith), fi = pi + 2 * gen;
  if (h->fused.mask[fi] == h->active_mask) return ANI_OK;
  free_fused(h, fi);
  const HostModel& m = h->model;
  const int M = m.M, acols = h->ap_run.aev_len, ka = h->ap_run.aev_stride;
  const int ks0 = acols / 16, nt0 = (acols + 31) / 32;
  for (int s = 0; s < m.S; s++) {
    SpeciesNet& n = h->nets[s];
    const std::vector<int>& d = m.dims[s];
    const int shape = fused_shape_for(d[1], d[2], d[3]);
    n.fused_shape = shape;
    int nt[3];
    fused_shape_tiles(shape, nt);
    SpeciesNet::Fused& f = n.fu[fi];
    f.ppm = gen ? fused16_pieces_per_member(shape, acols, P) : fused_pieces_per_member(shape, acols, P);
    f.cpm = fused_consts_floats(shape);
    HIP_TRY(h, hipMalloc((void**)&f.stream, (size_t)f.ppm * M * 1024));
    HIP_TRY(h, hipMalloc((void**)&f.consts, sizeof(float) * (size_t)f.cpm * M));
    std::vector<float> cst((size_t)f.cpm * M, 0.f);
    for (int a = 0; a < M; a++) {
      unsigned short* dst = reinterpret_cast<unsigned short*>(f.stream + (size_t)a * f.ppm * 1024);
      const float ws0 = n.wscale[0], ws1 = n.wscale[1], ws2 = n.wscale[2];
      if (!gen) {
        auto emit = [&](const float* src, int ld, int rows, int kval, int NT, int KS, int chunk, float scale) {
          launch_build_stream(src, ld, rows, kval, NT, KS, chunk, P, scale, dst, st);
          dst += (size_t)NT * KS * P * 512;
        };
        emit((n.W0c ? n.W0c : n.W[0]) + (size_t)a * d[1] * ka, ka, d[1], acols, nt[0], ks0, 0, ws0);                 // F1
        emit(n.W[1] + (size_t)a * d[2] * n.w[1], n.w[1], d[2], d[1], nt[1], 2 * nt[0], 0, ws1);                       // F2
        emit(n.W[2] + (size_t)a * d[3] * n.w[2], n.w[2], d[3], d[2], nt[2], 2 * nt[1], 0, ws2);                       // F3
        emit(n.WT[2] + (size_t)a * d[2] * n.w[3], n.w[3], d[2], d[3], nt[1], 2 * nt[2], -1, ws2);                     // B3
        emit(n.WT[1] + (size_t)a * d[1] * n.w[2], n.w[2], d[1], d[2], nt[0], 2 * nt[1], -1, ws1);                     // B2
        emit((n.WT0c ? n.WT0c : n.WT[0]) + (size_t)a * n.w[1], M * n.w[1], acols, d[1], nt0, 2 * nt[0], 4, ws0);      // B1 (chunks of kChunk tiles)
      } else {
        // the 16-row kernel's order (ani_kernels_mlpg.hip): 16-feature output tiles, 32-deep k-steps
        const int n1 = 2 * nt[0], n2 = 2 * nt[1], n3 = 2 * nt[2], ks1 = (acols + 31) / 32, nt16 = (acols + 15) / 16;
        auto emit = [&](const float* src, int ld, int rows, int kval, int NT, int KS, int order, int nt_off, int identity, float scale) {
          launch_build_stream16(src, ld, rows, kval, NT, KS, order, nt_off, identity, P, scale, dst, st);
          dst += (size_t)NT * KS * P * 512;
        };
        emit((n.W0c ? n.W0c : n.W[0]) + (size_t)a * d[1] * ka, ka, d[1], acols, n1, ks1, 0, 0, 1, ws0);               // F1: a slab per k-step
        emit(n.W[1] + (size_t)a * d[2] * n.w[1], n.w[1], d[2], d[1], n2, n1 / 2, 0, 0, 0, ws1);                       // F2
        emit(n.W[2] + (size_t)a * d[3] * n.w[2], n.w[2], d[3], d[2], n3, n2 / 2, 0, 0, 0, ws2);                       // F3
        emit(n.WT[2] + (size_t)a * d[2] * n.w[3], n.w[3], d[2], d[3], n2, n3 / 2, 1, 0, 0, ws2);                      // B3: tile-major
        emit(n.WT[1] + (size_t)a * d[1] * n.w[2], n.w[2], d[1], d[2], n1, n2 / 2, 1, 0, 0, ws1);                      // B2
        for (int ci = 0, c0 = 0; ci < fused16_b1_chunks(nt16); ci++) {                                                // B1: chunks of tiles
          const int ntc = fused16_b1_chunk_tiles(nt16, ci);
          emit((n.WT0c ? n.WT0c : n.WT[0]) + (size_t)a * n.w[1], M * n.w[1], acols, d[1], ntc, n1 / 2, 0, c0, 0, ws0);
          c0 += ntc;
        }
      }
      if ((size_t)(dst - reinterpret_cast<unsigned short*>(f.stream + (size_t)a * f.ppm * 1024)) != (size_t)f.ppm * 512) {
        h->err = "internal: fused MLP stream size mismatch";
        return ANI_ERR_MODEL;
      }
      float* c = cst.data() + (size_t)a * f.cpm;
      int off = 0;
      for (int o = 0; o < d[1]; o++) c[off + o] = m.b[a][s][0][o];
      off += 32 * nt[0];
      for (int o = 0; o < d[2]; o++) c[off + o] = m.b[a][s][1][o];
      off += 32 * nt[1];
      for (int o = 0; o < d[3]; o++) c[off + o] = m.b[a][s][2][o];
      off += 32 * nt[2];
      for (int o = 0; o < d[3]; o++) c[off + o] = m.W[a][s][3][o];
      off += 32 * nt[2];
      c[off] = m.b[a][s][3][0];
      const bool f16 = arith == MLP_F16X2;
      c[off + 1] = f16 ? 1.f / (16.f * ws0) : 1.f;
      c[off + 2] = f16 ? 1.f / (16.f * ws1) : 1.f;
      c[off + 3] = f16 ? 1.f / (16.f * ws2) : 1.f;
      c[off + 4] = f16 ? 1.f / (4096.f * ws2) : 1.f;
      c[off + 5] = f16 ? 1.f / (4096.f * ws1) : 1.f;
      c[off + 6] = f16 ? 1.f / (4096.f * ws0) : 1.f;
    }
    HIP_TRY(h, hipMemcpyAsync(f.consts, cst.data(), sizeof(float) * cst.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipStreamSynchronize(st));   // cst is a local
  }
  HIP_TRY(h, hipGetLastError());
  h->fused.mask[fi] = h->active_mask;
  return ANI_OK;
}

// The 16-row kernel: 128-row tiles on eight waves (two per SIMD) where that fills the CUs, else 64-row tiles on four -- twice
// the workgroups, about half the latency of a tile (a decomposed box's per-GPU share: 12 501 water atoms are 99 tiles of 128).
// Returns the 64-row tiles per 128-row tile: 2 or 1.
int fused_sub_tiles(const ani_handle* h) {
  const HostModel& m = h->model;
  if (!h->opt.mlp_fused_gen) return 1;
  int tiles128 = 0;
  for (int s = 0; s < m.S; s++) tiles128 += round_up(h->count[s], kRowTile) / kRowTile;
  const int items128 = tiles128 * (m.M > 1 && (h->opt.mlp_fused != 3 || h->armed.dv_force) ? m.M : 1);
  // 64-row tiles only where they still fit one round (a tile of either form costs about the same time per row)
  const bool small = h->opt.mlp_fused_rows == 64 || (h->opt.mlp_fused_rows == 0 && 2 * items128 <= device_num_cus() + device_num_cus() / 8);
  return small ? 2 : 1;
}

// the launch's arguments but for the schedule: the problems (species buckets, costliest first), tile_start, member_items, gaev_parts
int fill_fused_args(ani_handle* h, int fi, int sub, FusedArgs& G) {
  const HostModel& m = h->model;
  HIP_TRY(h, h->fused.counter.reserve(1));
  G.M = m.M; G.alpha = (float)m.alpha; G.inv_alpha = (float)(1.0 / m.alpha); G.scale = 1.f / (float)m.M;
  G.counter = h->fused.counter.p;
  G.err_flag = h->err_flag.p;
  const int acols = h->ap_run.aev_len, ka = h->ap_run.aev_stride;
  int np = 0, total = 0;
  for (int shape = 0; shape < kNumFusedShapes; shape++)        // costliest species first
    for (int s = 0; s < m.S; s++) {
      const SpeciesNet& n = h->nets[s];
      if (h->count[s] == 0 || n.fused_shape != shape) continue;
      if (np == kMaxProblems) { h->err = "too many species buckets for one fused MLP launch"; return ANI_ERR_ARG; }
      FusedProb& p = G.p[np];
      p.aev = h->aev.p + (size_t)h->row_start[s] * ka;
      p.gaev = h->gaev.p + (size_t)h->row_start[s] * ka;
      p.gaev_row0 = h->row_start[s];
      p.e_rows = h->e_rows.p + h->row_start[s];
      p.centre_of_row = h->centre_of_row.p + h->row_start[s];
      p.stream = n.fu[fi].stream; p.consts = n.fu[fi].consts;
      p.sE = h->nrows;
      p.tiles = sub * (round_up(h->count[s], kRowTile) / kRowTile);
      p.shape = shape;
      p.ks0 = acols / 16; p.nt0 = (acols + 31) / 32; p.acols = acols; p.aev_stride = ka;
      p.pieces_per_member = (int)n.fu[fi].ppm; p.consts_per_member = n.fu[fi].cpm;
      G.tile_start[np] = total;
      total += p.tiles;
      np++;
    }
  G.tile_start[np] = total;
  G.nprob = np;
  // Several members: a work item is (tile, member) -- M times the parallelism, and an even finish -- each member writing its
  // own dE/dAEV rows, summed by one small kernel (MLP ms, exact arithmetic, 8 members, against the grouped per-layer launches:
  // 10 002 water atoms 0.250 / 0.453, 25 002: 0.543 / 0.818, 50 001: 0.995 / 1.578, CH4/O2 100 008 (ANI-1x): 1.65 / 2.03; a
  // tile's members one after the other in its workgroup: 0.608 at 10 002 atoms).  The copies cost M times the dE/dAEV array:
  // beyond 8 GB the members run in sequence instead.
  const size_t parts_bytes = (size_t)std::max(h->nrows, 1) * ka * sizeof(float) * m.M;
  G.member_items = (m.M > 1 && parts_bytes <= ((size_t)8 << 30) && h->opt.mlp_fused != 3) ? 1 : 0;
  if (h->armed.dv_force) {   // a model-deviation step needs every member's rows: (tile, member) items whatever the option says
    if (parts_bytes > ((size_t)8 << 30)) {
      h->err = "ani_request_model_deviation: the per-member dE/dAEV rows of this step would take more than 8 GB";
      return ANI_ERR_ARG;
    }
    G.member_items = 1;
  }
  if (G.member_items) {
    const size_t per = (size_t)std::max(h->nrows, 1) * ka;
    HIP_TRY(h, h->fused.gaev_parts.reserve(per * m.M));
    G.gaev_parts = h->fused.gaev_parts.p;
    G.part_stride = (long long)per;
  }
  return ANI_OK;
}

// ANI_FUSED_SPLIT (experiments): "k0,k1,..." = how many of each type's last items the schedule cuts in two, types not named
// keep 0.  Returns split (filled), or null when the variable is not set.
const int* forced_fused_split(const char* env, int ntypes, const int* count, int* split) {
  if (!env) return nullptr;
  std::fill(split, split + ntypes, 0);
  int j = 0;
  for (const char* q = env; *q && j < ntypes; j++) {
    split[j] = std::max(0, std::min(count[j], atoi(q)));
    while (*q && *q != ',') q++;
    if (*q == ',') q++;
  }
  return split;
}

// a schedule (n items, then bins + 1 offsets) -> h->fused.sched
int upload_fused_schedule(ani_handle* h, const std::vector<int>& items, int n, const std::vector<int>& off, size_t cap, hipStream_t st) {
  HIP_TRY(h, h->fused.sched.reserve(cap));
  HIP_TRY(h, hipMemcpyAsync(h->fused.sched.p, items.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
  HIP_TRY(h, hipMemcpyAsync(h->fused.sched.p + n, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(h, hipStreamSynchronize(st));   // items / off are the caller's locals; once per re-neighbouring
  h->fused.sched_nitems = n;
  return ANI_OK;
}

// ms of two launches of the sixteen-row kernel on 128-row tiles with the schedule in h->fused.sched (a first one is not counted)
int time_fused_schedule(ani_handle* h, FusedArgs& G, MlpArith arith, int bins, hipStream_t st, float* ms) {
  G.sched_items = h->fused.sched.p; G.sched_off = h->fused.sched.p + h->fused.sched_nitems; G.sched_blocks = bins;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(h, hipEventCreate(&e0));
  HIP_TRY(h, hipEventCreate(&e1));
  hipError_t err = launch_mlp_fused16(G, arith, 8, st);
  if (err == hipSuccess) err = hipEventRecord(e0, st);
  for (int k = 0; k < 2 && err == hipSuccess; k++) err = launch_mlp_fused16(G, arith, 8, st);
  if (err == hipSuccess) err = hipEventRecord(e1, st);
  if (err == hipSuccess) err = hipEventSynchronize(e1);
  if (err == hipSuccess) err = hipEventElapsedTime(ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  HIP_TRY(h, err);
  return ANI_OK;
}

// Which workgroup runs which items: a static schedule in h->fused.sched, remade when the tile counts change (re-neighbouring);
// G.sched_* are pointed at it.
int ensure_fused_schedule(ani_handle* h, FusedArgs& G, MlpArith arith, int gen, int sub, hipStream_t st) {
  static const double half_cost = [] { const char* e = getenv("ANI_FUSED_HALF_COST"); return e ? atof(e) : kFusedHalfCost; }();
  static const bool autotune = [] { const char* e = getenv("ANI_FUSED_AUTOTUNE"); return !(e && atoi(e) == 0); }();
  const bool verbose = getenv("ANI_FUSED_AUTOTUNE_VERBOSE") != nullptr;
  const char* split_env = getenv("ANI_FUSED_SPLIT");
  const int np = G.nprob, total = G.tile_start[np], per_tile = G.member_items ? G.M : 1, bins = device_num_cus();
  const int nitems = total * per_tile;
  int mix = np;   // the tile counts and shapes of the problems, folded into one word
  for (int q = 0; q < np; q++) mix = mix * 1000003 + G.p[q].tiles * 4 + G.p[q].shape;
  mix = mix * 31 + sub + 2 * gen + 4 * h->opt.mlp_fused_halves;
  if (h->fused.sched_key[0] != total || h->fused.sched_key[1] != per_tile || h->fused.sched_key[2] != mix || h->fused.sched_key[3] != bins || !h->fused.sched.p) {
    // item types: one per problem; a (tile, member) item costs what its tile's member costs.  Item t of the kernel's numbering
    // is tile t / per_tile: the items of a problem are contiguous.
    int cnt[kMaxProblems], forced[kMaxProblems];
    double cost[kMaxProblems];
    for (int q = 0; q < np; q++) {
      int nt[3];
      fused_shape_tiles(G.p[q].shape, nt);
      cnt[q] = G.p[q].tiles * per_tile;
      cost[q] = (double)G.p[q].ks0 * nt[0] + 4.0 * nt[0] * nt[1] + 4.0 * nt[1] * nt[2] + 2.0 * nt[0] * G.p[q].nt0 +
                12.0;   // MFMA blocks of a member + a little for what a tile costs whatever its size
      if (!G.member_items) cost[q] *= G.M;
    }
    const int* forced_split = forced_fused_split(split_env, np, cnt, forced);
    // The sixteen-row kernel takes half items: the schedule may cut the items of a last, mostly idle round in two.  A half costs
    // about kFusedHalfCost of its item (64 of 128 rows with all the weights streamed: profiles/r04_mlp_halves.log), and the
    // cost model is good to about 5 %: a split the model likes by at least 3 % is TIMED against the whole items on this very
    // step's rows (three launches each, the first not counted; the launch is idempotent) and kept only if it is faster --
    // once per set of tile counts (ANI_FUSED_AUTOTUNE=0: no timing, a split needs 8 % by the model).
    const size_t cap = (size_t)2 * std::max(nitems, 1) + bins + 1;
    std::vector<int> items((size_t)2 * std::max(nitems, 1)), off(bins + 1), split(np, 0);
    int nsched = nitems;
    const int split_mode = !gen ? 0 : (h->opt.mlp_fused_halves == 2 ? 2 : (sub != 2 ? h->opt.mlp_fused_halves : 0));   // searched for 128-row tiles only
    (void)fused_schedule_halves(np, cnt, cost, half_cost, bins, split_mode, forced_split, split.data(), items.data(), off.data(), &nsched,
                                autotune && split_mode == 1 ? 0.03 : 0.08);
    int any_split = 0;
    for (int q = 0; q < np; q++) any_split += split[q];
    int rc = upload_fused_schedule(h, items, nsched, off, cap, st);
    if (rc) return rc;
    if (autotune && split_mode == 1 && any_split && !forced_split) {
      float t_split = 0.f, t_whole = 0.f;
      rc = time_fused_schedule(h, G, arith, bins, st, &t_split);
      if (rc) return rc;
      std::vector<int> items_w((size_t)std::max(nitems, 1)), off_w(bins + 1);
      int n_w = nitems;
      (void)fused_schedule_halves(np, cnt, cost, half_cost, bins, 0, nullptr, nullptr, items_w.data(), off_w.data(), &n_w);
      rc = upload_fused_schedule(h, items_w, n_w, off_w, cap, st);
      if (!rc) rc = time_fused_schedule(h, G, arith, bins, st, &t_whole);
      if (!rc && t_split < t_whole) rc = upload_fused_schedule(h, items, nsched, off, cap, st);   // the split stays: back it goes
      if (rc) return rc;
      if (verbose)
        fprintf(stderr, "libani_hip: fused MLP schedule, %d items: whole %.4f ms, with half items %.4f ms per launch -> %s\n", nitems,
                t_whole / 2, t_split / 2, t_split < t_whole ? "halves" : "whole");
    }
    h->fused.sched_key[0] = total; h->fused.sched_key[1] = per_tile; h->fused.sched_key[2] = mix; h->fused.sched_key[3] = bins;
  }
  G.sched_items = h->fused.sched.p;
  G.sched_off = h->fused.sched.p + h->fused.sched_nitems;
  G.sched_blocks = bins;
  return ANI_OK;
}

// the launch, then the members' dE/dAEV copies -> the step's
int launch_fused(ani_handle* h, const FusedArgs& G, MlpArith arith, int gen, int sub, hipStream_t st) {
  if (gen) {
    HIP_TRY(h, launch_mlp_fused16(G, arith, sub == 2 ? 4 : 8, st));
    h->last_mlp_kernel = arith == MLP_F16X2 ? (sub == 2 ? "mlp_fused16<2, 4>" : "mlp_fused16<2, 8>") : (sub == 2 ? "mlp_fused16<3, 4>" : "mlp_fused16<3, 8>");
  } else {
    HIP_TRY(h, launch_mlp_fused(G, arith, st));
    h->last_mlp_kernel = arith == MLP_F16X2 ? "mlp_fused<2>" : "mlp_fused<3>";
  }
  const long long n = (long long)h->nrows * h->ap_run.aev_stride;
  if (G.member_items && h->armed.dv_force) launch_dev_parts(h->fused.gaev_parts.p, G.part_stride, G.M, h->gaev.p, n, /*sum=*/1, st);
  else if (G.member_items) launch_sum_parts(h->fused.gaev_parts.p, G.part_stride, G.M, h->gaev.p, n, st);
  return ANI_OK;
}

int compute_mlp_fused(ani_handle* h, hipStream_t st) {
  const MlpArith arith = (MlpArith)h->opt.mlp_arith;
  const int gen = h->opt.mlp_fused_gen ? 1 : 0, fi = (arith == MLP_F16X2 ? 1 : 0) + 2 * gen;
  int rc = ensure_fused(h, arith, gen, st);
  if (rc) return rc;
  const int sub = fused_sub_tiles(h);
  FusedArgs G{};
  rc = fill_fused_args(h, fi, sub, G);
  if (!rc && h->opt.mlp_fused_sched) rc = ensure_fused_schedule(h, G, arith, gen, sub, st);
  if (!rc) rc = launch_fused(h, G, arith, gen, sub, st);
  return rc;
}

// The MLP ensemble for every species bucket, one grouped launch per layer (all species and members together).
// Buffers of species s are local to the bucket (row 0 = row_start[s]).
//   W[k]  : [M][d[k+1]][w[k]]   Bt of forward layer k (K = w[k], zero padded)
//   WT[k] : [M][d[k]][w[k+1]]   Bt of the backward product through layer k (k >= 1);  WT[0]: [aev_len][M*w[1]]
//   H_k   : [rows][M*w[k]]      activations after layer k-1 (member a at column a*w[k]); overwritten by G_k = dE/dz_k
int compute_mlp(ani_handle* h, hipStream_t st) {
  if (fused_eligible(h)) return compute_mlp_fused(h, st);
  {
    const int rca = ensure_arena(h, st);
    if (rca) return rca;
  }
  const HostModel& m = h->model;
  const int L = m.L, M = m.M;
  const float alpha = (float)m.alpha, inv_alpha = (float)(1.0 / m.alpha);
  std::vector<GemmArgs> probs;
  probs.reserve(m.S);
  // every layer's problems and epilogue, in launch order: either six grouped launches or one chained launch
  std::vector<std::vector<GemmArgs>> layer_probs;
  std::vector<int> layer_epi;
  const MlpArith arith = (MlpArith)h->opt.mlp_arith;
  const int spi = arith == MLP_F16X2 ? 1 : 0;
  // two-term fp16 path: power-of-two scales of the A operands (ani_kernels_mlp.hip): activations 2^4, gradients 2^12
  const float a_fwd = arith == MLP_F16X2 ? 16.f : 1.f, a_bwd = arith == MLP_F16X2 ? 4096.f : 1.f;
  auto set_planes = [&](GemmArgs& g, const unsigned short* planes, long long per_batch_matrices, float a_scale, float wscale) {
    g.Btp = planes; g.kbp = (g.K + 15) / 16;
    g.sBp = per_batch_matrices ? (long long)split_elems(g.N, g.K, arith) : 0;
    g.a_scale = a_scale;
    g.inv_scale = arith == MLP_F16X2 ? 1.f / (a_scale * wscale) : 1.f;
  };
  auto base_args = [&](int s) {
    GemmArgs g{};
    g.rows = round_up(h->count[s], kRowTile);
    g.row0 = 0;
    g.batch = M;
    g.alpha = alpha;
    g.inv_alpha = inv_alpha;
    g.scale = 1.f / (float)M;
    g.centre_of_row = h->centre_of_row.p + h->row_start[s];
    return g;
  };
  // forward
  for (int k = 0; k <= L - 2; k++) {
    probs.clear();
    for (int s = 0; s < m.S; s++) {
      if (h->count[s] == 0) continue;
      const SpeciesNet& n = h->nets[s];
      const std::vector<int>& d = m.dims[s];
      GemmArgs g = base_args(s);
      if (k == 0) {
        const int ka = h->ap_run.aev_stride;  // first layer over the AEV columns of the species present
        g.A = h->aev.p + (size_t)h->row_start[s] * ka; g.lda = ka; g.sA = 0;
        g.K = ka; g.Bt = n.W0c ? n.W0c : n.W[0]; g.ldb = ka; g.sB = (long long)d[1] * ka;
      } else {
        g.A = h->Hbuf[s][k]; g.lda = M * n.w[k]; g.sA = n.w[k];
        g.K = n.w[k]; g.Bt = n.W[k]; g.ldb = n.w[k]; g.sB = (long long)d[k + 1] * n.w[k];
      }
      g.N = d[k + 1];
      set_planes(g, (k == 0 && n.W0c) ? n.sp[spi].W0c : n.sp[spi].W[k], 1, a_fwd, n.wscale[k]);
      g.bias = n.b[k]; g.sBias = d[k + 1];
      g.C = h->Hbuf[s][k + 1]; g.ldc = M * n.w[k + 1]; g.sC = n.w[k + 1];
      if (k == L - 2) {
        g.aux = n.w_out; g.sAux = n.w[L - 1];
        g.bias_last = n.b_out;
        g.e_out = h->e_rows.p + h->row_start[s]; g.sE = h->nrows;
      }
      probs.push_back(g);
    }
    layer_probs.push_back(probs); layer_epi.push_back(k == L - 2 ? EPI_LAST : EPI_CELU);
  }
  // backward: dE/dh_{k-1} = G_k W[k-1] with G_k = dE/dh_k * celu'(z_k).  The celu' factor of a layer is applied when
  // its raw gradient is staged as the A operand of the next product (Amask = the stored activation H_k), not in the
  // epilogue of the product that made it: the H loads then ride the prefetch pipeline instead of stalling the epilogue.
  // G_{L-1} comes fully formed out of the fused last forward layer.
  for (int k = L - 1; k >= 2; k--) {
    probs.clear();
    for (int s = 0; s < m.S; s++) {
      if (h->count[s] == 0) continue;
      const SpeciesNet& n = h->nets[s];
      const std::vector<int>& d = m.dims[s];
      GemmArgs g = base_args(s);
      g.A = (k == L - 1) ? h->Hbuf[s][k] : h->Gbuf[s][k];
      g.Amask = (k == L - 1) ? nullptr : h->Hbuf[s][k];
      g.lda = M * n.w[k]; g.sA = n.w[k]; g.K = n.w[k];
      g.Bt = n.WT[k - 1]; g.ldb = n.w[k]; g.sB = (long long)d[k - 1] * n.w[k];
      g.N = d[k - 1];
      set_planes(g, n.sp[spi].WT[k - 1], 1, a_bwd, n.wscale[k - 1]);
      g.C = h->Gbuf[s][k - 1]; g.ldc = M * n.w[k - 1]; g.sC = n.w[k - 1];
      probs.push_back(g);
    }
    layer_probs.push_back(probs); layer_epi.push_back(EPI_PLAIN);
  }
  // dE/dAEV = sum over members of G_1 W[0]  (members concatenated along K)
  probs.clear();
  for (int s = 0; s < m.S; s++) {
    if (h->count[s] == 0) continue;
    const SpeciesNet& n = h->nets[s];
    GemmArgs g = base_args(s);
    g.batch = 1;
    g.A = h->Gbuf[s][1]; g.Amask = h->Hbuf[s][1]; g.lda = M * n.w[1]; g.K = M * n.w[1];
    g.Bt = n.WT0c ? n.WT0c : n.WT[0]; g.ldb = M * n.w[1];
    g.N = h->ap_run.aev_len;
    set_planes(g, n.WT0c ? n.sp[spi].WT0c : n.sp[spi].WT[0], 0, a_bwd, n.wscale[0]);
    g.C = h->gaev.p + (size_t)h->row_start[s] * h->ap_run.aev_stride; g.ldc = h->ap_run.aev_stride;
    probs.push_back(g);
  }
  layer_probs.push_back(probs); layer_epi.push_back(EPI_PLAIN);

  // One ensemble member, split arithmetic -- three ways to launch the six products:
  //  * up to one round of chained workgroups (2 per CU; <= 512 64-row tiles = 32 000 water atoms): ONE chained launch, a
  //    workgroup takes its tile through all layers (mlp_chain_x3);
  //  * beyond (two-term arithmetic, layers no wider than 256): ONE launch of persistent workgroups over (layer, tile) items
  //    with a completion flag per item (mlp_pipeline_x2) -- measured against the alternatives, MLP ms: 50 001 atoms 0.149
  //    (chained 0.203), 75 000 0.206 (grouped 0.240), 100 002 0.281 (grouped 0.320); 25 002 atoms 0.113 against 0.095
  //    chained;
  //  * otherwise one grouped launch per layer (several members, the exact bf16 split with many tiles, wide layers).
  const int np = (int)layer_probs[0].size();
  int tiles = 0;
  for (const GemmArgs& g : layer_probs[0]) tiles += g.rows / 64;
  const int cslots = mlp_chain_slots(), lslots = cslots + cslots / 2;
  bool pipeline = h->opt.mlp_pipeline && arith == MLP_F16X2 && M == 1 && np > 0 && (tiles > cslots || h->opt.mlp_pipeline > 1) &&
                  h->opt.mlp_chain <= 1;
  for (const auto& lp : layer_probs) {
    pipeline = pipeline && (int)lp.size() == np;
    for (const GemmArgs& g : lp)
      pipeline = pipeline && g.N <= 256 && g.batch == 1 && (g.ldc & 31) == 0 && (reinterpret_cast<uintptr_t>(g.C) & 127) == 0;
  }
  // without the pipeline the choice between chain and grouped launches is a matter of rounds (0.106 ms per chained round,
  // 0.137 ms per round of six grouped launches at the benchmark shapes)
  const bool chain_wins = tiles <= cslots || (tiles <= 2 * cslots &&
                                              0.106 * ((tiles + cslots - 1) / cslots) < 0.137 * ((tiles + lslots - 1) / lslots));
  bool chain = !pipeline && h->opt.mlp_chain && arith != MLP_FP32 && M == 1 && np > 0 && (h->opt.mlp_chain > 1 || chain_wins);
  for (const auto& lp : layer_probs) chain = chain && (int)lp.size() == np;
  if (chain || pipeline) {
    std::vector<GemmArgs> flat;
    for (const auto& lp : layer_probs) flat.insert(flat.end(), lp.begin(), lp.end());
    HIP_TRY(h, launch_mlp_chain(flat.data(), layer_epi.data(), (int)layer_probs.size(), np, &h->chain_plan, st, arith, pipeline,
                                h->err_flag.p));
    h->last_mlp_kernel = pipeline ? "mlp_pipeline" : "mlp_chain";
  } else {
    h->last_mlp_kernel = "gemm_grouped (one launch per layer)";
    for (size_t l = 0; l < layer_probs.size(); l++)
      launch_gemm_group(layer_probs[l].data(), (int)layer_probs[l].size(), (Epilogue)layer_epi[l], st, arith);
  }
  if (h->armed.dv_force && M > 1) {
    // model-deviation step: every member's own dE/dAEV rows, G_1 of member a (columns a w[1]) times its slice of WT[0], then
    // dg_m in place against the mean the product above wrote.  The split planes of WT[0] are blocked by 16 k: a member's slice
    // is a whole number of blocks when w[1] is a multiple of 16, else the product runs in fp32.
    const int ka = h->ap_run.aev_stride;
    const size_t per = (size_t)std::max(h->nrows, 1) * ka;
    HIP_TRY(h, h->fused.gaev_parts.reserve(per * M, true));
    bool planes = arith != MLP_FP32;
    for (int s = 0; s < m.S; s++) planes = planes && (h->count[s] == 0 || h->nets[s].w[1] % 16 == 0);
    probs.clear();
    for (int s = 0; s < m.S; s++) {
      if (h->count[s] == 0) continue;
      const SpeciesNet& n = h->nets[s];
      GemmArgs g = base_args(s);
      g.A = h->Gbuf[s][1]; g.Amask = h->Hbuf[s][1]; g.lda = M * n.w[1]; g.sA = n.w[1]; g.K = n.w[1];
      g.Bt = n.WT0c ? n.WT0c : n.WT[0]; g.ldb = M * n.w[1]; g.sB = n.w[1];
      g.N = h->ap_run.aev_len;
      if (planes) {
        set_planes(g, n.WT0c ? n.sp[spi].WT0c : n.sp[spi].WT[0], 0, a_bwd, n.wscale[0]);
        g.sBp = (long long)(n.w[1] / 16) * g.N * mlp_planes(arith) * 16;
      }
      g.C = h->fused.gaev_parts.p + (size_t)h->row_start[s] * ka; g.ldc = ka; g.sC = (long long)per;
      probs.push_back(g);
    }
    launch_gemm_group(probs.data(), (int)probs.size(), EPI_PLAIN, st, planes ? arith : MLP_FP32);
    launch_dev_parts(h->fused.gaev_parts.p, (long long)per, M, h->gaev.p, (long long)h->nrows * ka, /*sum=*/0, st);
  }
  return ANI_OK;
}
}  // namespace ani_host
