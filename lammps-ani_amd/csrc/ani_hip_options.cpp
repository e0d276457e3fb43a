// ani_hip_options.cpp — ani_set_option, the ani_debug_* views, timeline markers, phase timing.  Internal: see ani_handle.h.
#include "ani_handle.h"

extern "C" {
void ani_trace_push(const char* name) { if (name) roctxRangePushA(name); }
void ani_trace_pop(void) { roctxRangePop(); }
void ani_trace_mark(const char* name) { if (name) roctxMarkA(name); }

const char* ani_last_mlp_kernel(const ani_handle* h) { return h ? h->last_mlp_kernel : ""; }
const char* ani_last_repulsion_kernel(const ani_handle* h) { return h ? h->last_rep_kernel : ""; }

int ani_debug_get(ani_handle* h, ani_debug_view* out) {
  if (!h || !out) return ANI_ERR_ARG;
  memset(out, 0, sizeof(*out));
  out->nlocal = h->nlocal; out->ntotal = h->ntotal; out->nrows = h->nrows; out->npairs = h->npairs;
  out->d_aev = h->aev.p; out->d_gaev = h->gaev.p; out->d_row_of_centre = h->row_of_centre.p;
  out->aev_stride = h->ap_run.aev_stride; out->aev_active_length = h->ap_run.aev_len;
  if (h->err_flag.p) {   // a diagnostics call: wait for whatever is queued on the device, then read the word as it stands
    int flag = 0;
    if (hipSetDevice(h->device) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
        hipMemcpy(&flag, h->err_flag.p, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
      h->sticky_flags |= flag;
  }
  out->error_flags = h->sticky_flags;
  for (int s = 0; s < kMaxSpecies && s < 16; s++) out->species_count[s] = h->count[s];
  return ANI_OK;
}

int ani_debug_deviation_parts(ani_handle* h, const void** d_parts, int64_t* member_stride) {
  if (!h || !d_parts || !member_stride) return ANI_ERR_ARG;
  *d_parts = h->use_single ? static_cast<const void*>(h->fused.gaev_parts.p) : static_cast<const void*>(h->armed.gaev_parts64.p);
  *member_stride = (int64_t)std::max(h->nrows, 1) * h->ap_run.aev_stride;
  return ANI_OK;
}

int ani_debug_list(ani_handle* h, const int** d_numneigh, const int** d_nbr_off, const int** d_jlist) {
  if (!h || !h->have_list) return ANI_ERR_ARG;
  if (d_numneigh) *d_numneigh = h->numneigh.p;
  if (d_nbr_off) *d_nbr_off = h->nbr_off.p;
  if (d_jlist) *d_jlist = h->jlist.p;   // the installed list: every centre's segment grouped by neighbour species
  return ANI_OK;
}

int ani_debug_stream_tables(ani_handle* h, ani_stream_tables_view* view, int32_t* desc_bwd, uint32_t* words_bwd, int32_t* desc_fwd,
                            uint32_t* words_fwd) {
  if (!h || !view) return ANI_ERR_ARG;
  memset(view, 0, sizeof(*view));
  const StreamTables& t = h->stab;
  view->builds = t.builds;
  view->build_ms = t.build_ms;
  if (t.S == 0 || t.mask != h->active_mask) return ANI_OK;   // no tables for the layout of the epoch
  view->species = t.S; view->bound = t.nt; view->tuples = t.tuples;
  view->words_bwd = (int64_t)t.nwords_b; view->words_fwd = (int64_t)t.nwords_f;
  view->d_words_bwd = t.words_b.p; view->d_words_fwd = t.words_f.p;
  if (!desc_bwd && !words_bwd && !desc_fwd && !words_fwd) return ANI_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (desc_bwd) HIP_TRY(h, hipMemcpy(desc_bwd, t.desc_b.p, sizeof(int4) * t.tuples, hipMemcpyDeviceToHost));
  if (desc_fwd) HIP_TRY(h, hipMemcpy(desc_fwd, t.desc_f.p, sizeof(int4) * t.tuples, hipMemcpyDeviceToHost));
  if (words_bwd && t.nwords_b) HIP_TRY(h, hipMemcpy(words_bwd, t.words_b.p, sizeof(unsigned) * t.nwords_b, hipMemcpyDeviceToHost));
  if (words_fwd && t.nwords_f) HIP_TRY(h, hipMemcpy(words_fwd, t.words_f.p, sizeof(unsigned) * t.nwords_f, hipMemcpyDeviceToHost));
  return ANI_OK;
}

int ani_debug_colmap(ani_handle* h, int* out) {
  if (!h || !out) return ANI_ERR_ARG;
  for (int c = 0; c < h->ap_run.aev_len && c < (int)h->colmap.size(); c++) out[c] = h->colmap[c];
  return ANI_OK;
}

// ani_set_option: one row per name.  A flag stores value != 0; a range accepts v[0] <= value <= v[1]; a set accepts the values
// v[0..2]; a value outside is refused with the row's text and changes nothing.  What a new value invalidates is cleared with it.
enum OptKind { kFlag, kRange, kSet };
enum OptInvalidates { kNothing, kSchedule, kList, kUpload };   // fused.sched_key[0] | have_list + active_mask | host.x64_from
struct OptRow { const char* name; int Options::*field; OptKind kind; int v[3]; const char* refusal; OptInvalidates invalidates; };   // field null: full_cap of both AEV layouts
constexpr int kAny = 0x7fffffff;
static const OptRow kOptionRows[] = {
    {"prune_absent_species", &Options::prune, kFlag, {}, nullptr, kList},   // takes effect at the next rebuild (ago = 0), which the caller must issue
    {"rdf_lanes", &Options::rdf_lanes, kSet, {16, 64, 64}, "ani_set_option: rdf_lanes is 16 or 64", kNothing},
    {"rdf_lds", &Options::rdf_lds, kFlag, {}, nullptr, kNothing},
    {"mlp_chain", &Options::mlp_chain, kRange, {-kAny - 1, kAny}, nullptr, kNothing},
    {"nbr_onepass", &Options::nbr_onepass, kFlag, {}, nullptr, kNothing},
    {"out_force_accumulate", &Options::out_force_accumulate, kFlag, {}, nullptr, kNothing},
    {"nbr_sorted_rows", &Options::nbr_sorted_rows, kFlag, {}, nullptr, kNothing},
    {"nbr_half_cells", &Options::nbr_half_cells, kFlag, {}, nullptr, kNothing},
    {"reuse_build_list_upload", &Options::reuse_upload, kFlag, {}, nullptr, kUpload},
    {"mlp_fused", &Options::mlp_fused, kRange, {0, 3}, "mlp_fused must be 0, 1, 2 or 3", kNothing},
    {"aev_symmetric_radial", &Options::aev_sym_radial, kFlag, {}, nullptr, kNothing},
    {"aev_tickets_min", &Options::aev_tickets_min, kRange, {0, kAny}, "aev_tickets_min must be >= 0", kNothing},
    {"aev_fused", &Options::aev_fused, kFlag, {}, nullptr, kNothing},
    {"aev_stream_tables", &Options::aev_stream_tables, kFlag, {}, nullptr, kNothing},
    {"mlp_fused_gen", &Options::mlp_fused_gen, kRange, {0, 1}, "mlp_fused_gen must be 0 or 1", kSchedule},
    {"mlp_fused_rows", &Options::mlp_fused_rows, kSet, {0, 64, 128}, "mlp_fused_rows must be 0, 64 or 128", kSchedule},
    {"mlp_fused_halves", &Options::mlp_fused_halves, kRange, {0, 2}, "mlp_fused_halves must be 0, 1 or 2", kSchedule},
    {"mlp_fused_schedule", &Options::mlp_fused_sched, kFlag, {}, nullptr, kSchedule},
    {"mlp_pipeline", &Options::mlp_pipeline, kRange, {0, 2}, "mlp_pipeline must be 0, 1 or 2", kNothing},
    {"mlp_arith", &Options::mlp_arith, kRange, {0, 2}, "mlp_arith must be 0 (fp32-input MFMA), 1 (bf16 x 3, exact) or 2 (fp16 x 2)", kNothing},
    {"mlp_split_bf16", &Options::mlp_arith, kFlag, {}, nullptr, kNothing},   // earlier name: 1 = the exact bf16 split, 0 = fp32-input MFMA
    {"device_overwrite_forces", &Options::dev_overwrite, kFlag, {}, nullptr, kNothing},
    {"profiling", &Options::profiling, kFlag, {}, nullptr, kNothing},
    {"full_radial_capacity", nullptr, kFlag, {}, nullptr, kNothing},
};
static_assert(MLP_FP32 == 0 && MLP_BF16X3 == 1, "mlp_split_bf16 is a flag onto mlp_arith");

int ani_set_option(ani_handle* h, const char* name, int value) {
  if (!h || !name) return ANI_ERR_ARG;
  for (const OptRow& r : kOptionRows) {
    if (strcmp(name, r.name) != 0) continue;
    const bool ok = r.kind == kFlag || (r.kind == kRange ? value >= r.v[0] && value <= r.v[1] : value == r.v[0] || value == r.v[1] || value == r.v[2]);
    if (!ok) { h->err = r.refusal; return ANI_ERR_ARG; }
    const int stored = r.kind == kFlag ? value != 0 : value;
    if (r.field) h->opt.*r.field = stored;
    else h->ap.full_cap = h->ap_run.full_cap = stored;
    if (r.invalidates == kSchedule) h->fused.sched_key[0] = -1;
    if (r.invalidates == kList) { h->have_list = false; h->active_mask = -1; }
    if (r.invalidates == kUpload) h->host.x64_from = nullptr;
    return ANI_OK;
  }
  h->err = std::string("unknown option '") + name + "'";
  return ANI_ERR_ARG;
}

// development probe (tools/mlpf_stamps.py): phase cycle counters of a -DABLF_STAMPS build of the fused MLP; 0 otherwise
int ani_debug_fused_stamps(unsigned long long* out32, int reset) {   // 1: fused MLP stamps, 2: AEV backward stamps, 0: neither built in
  const int r = fused_read_stamps(out32, reset);
  return r ? r : aev_read_stamps(out32, reset);
}

int ani_debug_fused_schedule_halves(int ntypes, const int* count, const double* cost, double half_ratio, int bins, int split_mode,
                                    int* split_out, int* items_out, int* off_out, int* n_items_out, double* makespan_out) {
  if (ntypes < 1 || ntypes > kMaxProblems || !count || !cost || bins < 1 || !items_out || !off_out || split_mode < 0 || split_mode > 2 ||
      !(half_ratio > 0.0))
    return ANI_ERR_ARG;
  for (int j = 0; j < ntypes; j++)
    if (count[j] < 0 || !(cost[j] > 0.0)) return ANI_ERR_ARG;
  int forced[kMaxProblems];
  const double T = fused_schedule_halves(ntypes, count, cost, half_ratio, bins, split_mode,
                                         forced_fused_split(getenv("ANI_FUSED_SPLIT"), ntypes, count, forced), split_out, items_out, off_out,
                                         n_items_out);
  if (makespan_out) *makespan_out = T;
  return ANI_OK;
}

int ani_debug_fused_schedule(int ntypes, const int* count, const double* cost, int bins, int* items_out, int* off_out,
                             double* makespan_out) {
  if (ntypes < 1 || ntypes > kMaxProblems || !count || !cost || bins < 1 || !items_out || !off_out) return ANI_ERR_ARG;
  for (int j = 0; j < ntypes; j++)
    if (count[j] < 0 || !(cost[j] > 0.0)) return ANI_ERR_ARG;
  (void)fused_schedule(ntypes, count, cost, bins, items_out, off_out);
  if (makespan_out) {
    std::vector<int> type_of;
    for (int j = 0; j < ntypes; j++) type_of.insert(type_of.end(), count[j], j);
    double worst = 0.0;
    for (int b = 0; b < bins; b++) {
      double load = 0.0;
      for (int i = off_out[b]; i < off_out[b + 1]; i++) load += cost[type_of[items_out[i]]];
      worst = std::max(worst, load);
    }
    *makespan_out = worst;
  }
  return ANI_OK;
}

int ani_debug_read(ani_handle* h, const void* d_src, void* host_dst, uint64_t bytes) {
  if (!h || !d_src || !host_dst) return ANI_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(host_dst, d_src, bytes, hipMemcpyDeviceToHost));
  return ANI_OK;
}

int ani_phase_timing(ani_handle* h, int enable) {
  if (!h) return ANI_ERR_ARG;
  h->timing.on = enable != 0;
  if (enable != 0 && h->timing.evt_pool.empty()) {
    // the first batch of events is made here, not inside the first step that records (a timed step of the caller)
    (void)hipSetDevice(h->device);
    h->timing.evt_pool.resize(6 * 64, nullptr);
    for (hipEvent_t& e : h->timing.evt_pool) HIP_TRY(h, hipEventCreate(&e));
  }
  if (enable == 1) {  // fresh accumulation; 0 (stop) and 2 (resume) keep what has been recorded
    for (double& v : h->timing.phase_ms) v = 0;
    h->timing.phase_calls = 0;
    h->timing.evt_used = 0;
  }
  return ANI_OK;
}

int ani_phase_times(ani_handle* h, double* ms5, int* ncalls) {
  if (!h || !ms5 || !ncalls) return ANI_ERR_ARG;
  // resolve the recorded-but-unread steps (the caller has synchronised, or we wait here for the last event)
  // events of a step: 0 start, 5 after pack + compaction, 1 after AEV forward, 2 after the MLP, 3 after AEV backward, 4 end
  for (size_t b = 0; b + 6 <= h->timing.evt_used; b += 6) {
    HIP_TRY(h, hipEventSynchronize(h->timing.evt_pool[b + 4]));
    float t;
    HIP_TRY(h, hipEventElapsedTime(&t, h->timing.evt_pool[b + 0], h->timing.evt_pool[b + 5])); h->timing.phase_ms[4] += t;
    HIP_TRY(h, hipEventElapsedTime(&t, h->timing.evt_pool[b + 5], h->timing.evt_pool[b + 1])); h->timing.phase_ms[0] += t;
    for (int i = 1; i < 4; i++) {
      HIP_TRY(h, hipEventElapsedTime(&t, h->timing.evt_pool[b + i], h->timing.evt_pool[b + i + 1]));
      h->timing.phase_ms[i] += t;
    }
    h->timing.phase_calls++;
  }
  h->timing.evt_used = 0;
  for (int i = 0; i < 5; i++) ms5[i] = h->timing.phase_ms[i];
  *ncalls = h->timing.phase_calls;
  return ANI_OK;
}
}  // extern "C"
